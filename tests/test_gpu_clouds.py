"""The node's point-cloud topics on the GPU (dsm_cloud_compose / dsm_frame_cloud, dsm_surfel_map_get_cloud* /
dsm_surfel_map_set_publish): every cloud bit-identical (as uint32, NaN payloads kept) to a numpy restatement of the
reference's publish_*_pointcloud statements (surfel_fusion/src/surfel_map.cpp:1115-1151, 1283-1454)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ALL_KINDS = ("active", "inactive", "all", "neighbor", "raw")


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


def _engine(api, w=64, h=32, cap=1 << 16, slots=2, fx=57.25, fy=55.5, cx=31.3, cy=15.7):
    ff = api.FusionFunctions()
    ff.initialize(w, h, fx, fy, cx, cy, 30.0, 0.3, surfel_capacity=cap, frame_slots=slots)
    return ff


def _xyzi(s):
    return np.stack([s["px"], s["py"], s["pz"], s["color"]], axis=1).astype(np.float32).reshape(-1, 4)


def _same(a, b, what=""):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 4)
    b = np.ascontiguousarray(b, np.float32).reshape(-1, 4)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.size:
        bad = np.nonzero((a.view("u4") != b.view("u4")).any(axis=1))[0]
        assert bad.size == 0, (what, int(bad[0]), a[bad[0]], b[bad[0]])


def _random_map(rng, n, ut=None):
    """records with arbitrary bit patterns in the published fields (NaN payloads, inf, denormals) and update_times from an
    adversarial set (negative, zero, the threshold, huge)"""
    from densesurfelmapping_amd import api
    a = np.zeros(n, api.SURFEL_DTYPE)
    raw = rng.integers(0, 1 << 32, size=(n, 11), dtype=np.uint64).astype(np.uint32)
    for k, f in enumerate(("px", "py", "pz", "nx", "ny", "nz", "size", "color", "weight")):
        a[f] = raw[:, k].view(np.float32)
    a["update_times"] = ut if ut is not None else rng.choice(np.array([0, 1, 4, 5, 6, -1, -5, 2**31 - 1, -2**31, 100], np.int32), n)
    a["last_update"] = rng.integers(0, 8, n)
    return a


def _expect(m, select):
    if select == 0:
        return np.zeros((0, 4), np.float32)
    keep = m["update_times"] >= 5 if select == 1 else m["update_times"] != 0
    return _xyzi(m[keep])


# ------------------------------------------------------------------ 1. map compaction
def test_compaction_golden_maps(api):
    for name in ("tiny_drive_48_final_map.npy", "vga_rgbd_4_final_map.npy", "kitti1226_drive_5_final_map.npy"):
        m = np.load(os.path.join(ROOT, "tests", "golden", name))
        ff = _engine(api, cap=max(len(m), 1))
        ff.map_upload(m)
        for sel in (api.CLOUD_SELECT_MATURE, api.CLOUD_SELECT_NONZERO, api.CLOUD_SELECT_NONE):
            _same(ff.cloud_compose(sel), _expect(m, sel), (name, sel))
        ff.close()


def test_compaction_edge_sizes(api):
    rng = np.random.default_rng(7)
    ff = _engine(api, cap=1 << 15)
    full = ff.map_capacity()
    T = api.CLOUD_TILE
    for n in (0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17, full - 1, full):
        m = _random_map(rng, n)
        ff.map_upload(m)
        for sel in (1, 2):
            _same(ff.cloud_compose(sel), _expect(m, sel), (n, sel))
    n = 5 * T + 3
    for name, ut in (("none pass", np.zeros(n, np.int32)), ("all pass", np.full(n, 7, np.int32)),
                     ("alternating", np.where(np.arange(n) % 2 == 0, 5, 4).astype(np.int32)),
                     ("every 64th", np.where(np.arange(n) % 64 == 63, 9, -3).astype(np.int32))):
        m = _random_map(rng, n, ut)
        ff.map_upload(m)
        for sel in (1, 2):
            _same(ff.cloud_compose(sel), _expect(m, sel), (name, sel))
    ff.close()


def test_compaction_large_map_order(api):
    """> 2 M records: the order across thousands of workgroups"""
    rng = np.random.default_rng(11)
    n = (1 << 21) + 4321
    ff = _engine(api, cap=n)
    m = _random_map(rng, n)
    ff.map_upload(m)
    for sel in (1, 2):
        _same(ff.cloud_compose(sel), _expect(m, sel), sel)
    ff.close()


def test_compaction_capacity_overflow(api):
    import torch
    rng = np.random.default_rng(3)
    ff = _engine(api, cap=1 << 14)
    m = _random_map(rng, 9000)
    ff.map_upload(m)
    exp = _expect(m, 1)
    need = len(exp)
    cap = need - 100
    lib = ff._lib
    n = C.c_int32(-1)
    host = np.full((cap + 64, 4), 12345.0, np.float32)
    rc = lib.dsm_cloud_compose(ff._h, 1, 0, None, None, host.ctypes.data_as(C.c_void_p), 0, cap, C.byref(n))
    assert rc == api.DSM_E_CAPACITY and n.value == need
    assert (host[cap:] == 12345.0).all()
    dev = torch.full((cap + 64, 4), 12345.0, dtype=torch.float32, device="cuda")
    n.value = -1
    rc = lib.dsm_cloud_compose(ff._h, 1, 0, None, None, C.c_void_p(dev.data_ptr()), 1, cap, C.byref(n))
    assert rc == api.DSM_E_CAPACITY and n.value == need
    d = dev.cpu().numpy()
    assert (d[cap:] == 12345.0).all()
    _same(d[:cap], exp[:cap], "prefix below cap")
    # exactly enough
    dev = torch.full((need, 4), 12345.0, dtype=torch.float32, device="cuda")
    assert ff.cloud_compose(1, dst_ptr=dev.data_ptr(), cap=need) == need
    _same(dev.cpu().numpy(), exp)
    ff.close()


# ------------------------------------------------------------------ 2. store runs
def test_segments(api):
    import torch
    rng = np.random.default_rng(5)
    ff = _engine(api, cap=1 << 15)
    m = _random_map(rng, 20000)
    m["last_update"] = rng.integers(0, 9, len(m))
    ff.map_upload(m)
    for key in (3, 0, 7, 5):
        ff.store_deactivate(key)
    store_n = ff.store_size()
    _, cloud = ff.store_download(0, store_n)
    live = ff.map_download()
    assert store_n > 0
    cases = [[], [(0, store_n)], [(5, 0), (0, 0)], [(store_n - 1, 1), (0, 3), (100, 50), (7, 0), (100, 50)],
             [(store_n - 10, 10)]]
    for _ in range(6):
        k = int(rng.integers(1, 12))
        b = rng.integers(0, store_n, k)
        c = [int(rng.integers(0, store_n - x + 1)) for x in b]
        cases.append(list(zip(b.tolist(), c)))
    for segs in cases:
        tail = np.concatenate([cloud[b:b + c] for b, c in segs]) if segs else np.zeros((0, 4), np.float32)
        for sel in (0, 1, 2):
            _same(ff.cloud_compose(sel, segs), np.concatenate([_expect(live, sel), tail]), (segs, sel))
        cap = len(live) + sum(c for _, c in segs)
        dev = torch.zeros((cap, 4), dtype=torch.float32, device="cuda")
        n = ff.cloud_compose(2, segs, dst_ptr=dev.data_ptr(), cap=cap)
        _same(dev.cpu().numpy()[:n], np.concatenate([_expect(live, 2), tail]), ("device", segs))
    for bad in ([(0, store_n + 1)], [(-1, 2)], [(store_n, 1)], [(3, -1)]):
        with pytest.raises(api.DsmError) as e:
            ff.cloud_compose(1, bad, cap=1 << 16)
        assert e.value.code == api.DSM_E_INVALID
    ff.close()


# ------------------------------------------------------------------ 3. raw back-projection
def _raw_expect(image, depth, pose7, fx, fy, cx, cy):
    """publish_raw_pointcloud (:1115-1151) in float32, operation by operation (numpy does not contract to FMA)"""
    f = np.float32
    h, w = depth.shape
    x, y, z, qw = (f(pose7[3]), f(pose7[4]), f(pose7[5]), f(pose7[6]))
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = [[f(1) - (tyy + tzz), txy - twz, txz + twy],
         [txy + twz, f(1) - (txx + tzz), tyz - twx],
         [txz - twy, tyz + twx, f(1) - (txx + tyy)]]
    T = [f(pose7[0]), f(pose7[1]), f(pose7[2])]
    i = np.arange(w, dtype=np.float32)[:, None]
    j = np.arange(h, dtype=np.float32)[None, :]
    d = depth.T.astype(np.float32)
    with np.errstate(all="ignore"):
        c = [((i - f(cx)) * d) / f(fx), ((j - f(cy)) * d) / f(fy), d]
        out = np.empty((w, h, 4), np.float32)
        for r in range(3):
            out[..., r] = (((R[r][0] * c[0] + R[r][1] * c[1]) + R[r][2] * c[2]) + T[r])
    out[..., 3] = image.T.astype(np.float32)
    return out.reshape(-1, 4)


def _adversarial_frame(rng, w, h):
    depth = rng.uniform(0.1, 40.0, (h, w)).astype(np.float32)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -3.5, 1e-40, -1e-42, 3e38], np.float32)
    mask = rng.random((h, w)) < 0.3
    depth[mask] = rng.choice(specials, int(mask.sum()))
    nan_payload = np.array([0x7fc12345, 0xffa00001], np.uint32).view(np.float32)
    depth.reshape(-1)[rng.integers(0, w * h, 5)] = rng.choice(nan_payload, 5)
    image = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return image, depth


def test_raw_cloud(api):
    import torch
    rng = np.random.default_rng(13)
    fx, fy, cx, cy = 57.25, 55.5, 31.3, 15.7
    for (w, h) in ((64, 32), (203, 77), (130, 33), (24, 25), (1226, 370)):
        ff = _engine(api, w=w, h=h, fx=fx, fy=fy, cx=cx, cy=cy)
        for slot in (0, 1):
            image, depth = _adversarial_frame(rng, w, h)
            ff.frame_upload(slot, image, depth)
            q = rng.normal(size=4) * rng.choice([1.0, 0.3, 2.7])  # random, not unit
            pose7 = np.concatenate([rng.normal(size=3) * 10, q])
            exp = _raw_expect(image, depth, pose7, fx, fy, cx, cy)
            _same(ff.frame_cloud(slot, pose7), exp, (w, h, slot))
            dev = torch.zeros((w * h, 4), dtype=torch.float32, device="cuda")
            assert ff.frame_cloud(slot, pose7, dst_ptr=dev.data_ptr(), cap=w * h) == w * h
            # a new frame into the slot right after the call leaves the cloud as it was
            image2, depth2 = _adversarial_frame(rng, w, h)
            ff.frame_upload(slot, image2, depth2)
            _same(dev.cpu().numpy(), exp, ("device", w, h, slot))
            _same(ff.frame_cloud(slot, pose7), _raw_expect(image2, depth2, pose7, fx, fy, cx, cy), ("after upload", w, h))
        with pytest.raises(api.DsmError) as e:
            ff.frame_cloud(0, pose7, cap=w * h - 1)
        assert e.value.code == api.DSM_E_CAPACITY
        ff.close()


# ------------------------------------------------------------------ 4.-6. the node
def _driftfree(links, root, rng_):
    """SurfelMap::get_driftfree_poses (:1643-1673)"""
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


def _clouds_from_taps(node, relative_index, drift_free_poses, frame, fuse_pose, cam):
    local = node.local_surfels()
    inactive = node.inactive_cloud()
    poses = [node.pose(i) for i in range(node.pose_count)]
    active = _xyzi(local[local["update_times"] >= 5])
    neighbor = [_xyzi(local[local["update_times"] != 0])]
    for p in _driftfree([pp["links"] for pp in poses], relative_index, 2 * drift_free_poses):
        if poses[p]["is_local"] or poses[p]["n_attached"] <= 0:
            continue
        b = poses[p]["points_begin_index"]
        neighbor.append(inactive[b:b + poses[p]["n_attached"]])
    image, depth = frame
    raw = _raw_expect(image, depth, fuse_pose, cam.fx, cam.fy, cam.cx, cam.cy)
    return {"active": active, "inactive": inactive, "all": np.concatenate([active, inactive]),
            "neighbor": np.concatenate(neighbor), "raw": raw}


def _run_publishing_node(case):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import node_state
    from densesurfelmapping_amd import surfel_map, synth
    cam, scene = node_state.camera_and_scene(case, synth)
    node = surfel_map.SurfelMap(cam, drift_free_poses=case["drift_free_poses"])
    frames, pubs, problems = {}, [], []

    def on_publish(pub):
        try:
            exp = _clouds_from_taps(node, pub["relative_index"], case["drift_free_poses"], frames[pub["stamp"]], pub["fuse_pose"], cam)
            for k in ALL_KINDS:
                _same(pub["clouds"][k], exp[k], (case["name"], len(pubs), k))
        except Exception as e:  # (exceptions do not cross the C callback: collect them)
            problems.append(repr(e))
        pubs.append(pub)

    node.set_publish(ALL_KINDS, on_publish)
    for ev in synth.node_messages(cam, scene, case["frames"], **case["kw"]):
        if ev[0] in ("image", "depth"):
            f = frames.setdefault(tuple(ev[1]), [None, None])
            f[0 if ev[0] == "image" else 1] = np.array(ev[2])
        node.feed(ev)
    return node, pubs, problems


def test_node_publications_per_fuse(api):
    import test_cpu
    for case, gold in test_cpu._node_cases():
        node, pubs, problems = _run_publishing_node(case)
        assert problems == [], problems[:3]
        assert len(pubs) == node.frames_fused > 0
        ref_final = np.load(os.path.join(ROOT, "tests", "golden", gold["final"]))
        local = ref_final["local"]
        ref_active = _xyzi(local[local["update_times"] >= 5])
        last = pubs[-1]["clouds"]
        _same(last["active"], ref_active, (case["name"], "active vs reference node"))
        _same(last["inactive"], ref_final["cloud"], (case["name"], "inactive vs reference node"))
        _same(last["all"], np.concatenate([ref_active, ref_final["cloud"]]), (case["name"], "all vs reference node"))
        # 6. the pull API returns the same as the last publication (nothing happened since)
        for k in ALL_KINDS:
            _same(node.cloud(k), last[k], (case["name"], "pull", k))
        node.close()


def test_node_publication_changes_nothing(api):
    """every brief, checkpoint, final state and export of the golden node run with all five clouds published"""
    import test_cpu
    from densesurfelmapping_amd import surfel_map
    seen = []

    def make(cam, d):
        node = surfel_map.SurfelMap(cam, drift_free_poses=d)
        node.set_publish(ALL_KINDS, lambda pub: seen.append(sum(len(c) for c in pub["clouds"].values())))
        return node

    for case, gold in test_cpu._node_cases():
        n0 = len(seen)
        test_cpu._check_node_run(case, gold, make)
        assert len(seen) > n0


def test_node_pull_api(api):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import node_state
    import test_cpu
    from densesurfelmapping_amd import surfel_map, synth
    case, _ = test_cpu._node_cases()[0]
    cam, scene = node_state.camera_and_scene(case, synth)
    node = surfel_map.SurfelMap(cam, drift_free_poses=case["drift_free_poses"])
    for k in ALL_KINDS:
        with pytest.raises(api.DsmError) as e:
            node.cloud(k)
        assert e.value.code == api.DSM_E_STATE
    for i, ev in enumerate(synth.node_messages(cam, scene, 24, **case["kw"])):
        node.feed(ev)
    assert node.frames_fused > 0
    for k in ALL_KINDS:
        host = node.cloud(k)
        cap = len(host) + 10
        dev = torch.full((cap, 4), -7.0, dtype=torch.float32, device="cuda")
        assert node.cloud_to_device(k, dev.data_ptr(), cap) == len(host)
        d = dev.cpu().numpy()
        _same(d[:len(host)], host, k)
        assert (d[len(host):] == -7.0).all()
        if len(host):
            with pytest.raises(api.DsmError) as e:
                node.cloud_to_device(k, dev.data_ptr(), len(host) - 1)
            assert e.value.code == api.DSM_E_CAPACITY
    node.set_publish((), None)  # off again
    node.close()
