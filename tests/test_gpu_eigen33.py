"""DSM_FLAG_EIGEN33_PRODUCTS on the GPU: every form of the frame pipeline with the flag reproduces the fixtures recorded from
the reference built against an Eigen >= 3.3 stand-in (tests/golden/make_golden_eigen33.py) byte for byte, NaN == NaN; the
same runs without the flag stay the Eigen 3.2 results; the node and its RAW cloud follow the flag."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, fields_equal

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def mods(oracle_built):
    import torch
    torch.cuda.init()  # torch's lazy HIP initialisation first, as in the other GPU suites
    import eigen33_cases
    from densesurfelmapping_amd import api, synth
    from oracle import bindings
    return api, synth, bindings, eigen33_cases


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLDEN, "eigen33_golden.json")))


def _case(gold, E, name):
    return next(c for c in E.SEQUENCES if c["name"] == name), next(g for g in gold["sequences"] if g["name"] == name)


def _check_final(tag, got, g):
    import eigen33_cases as E
    bad = E.final_map_differences(got, g, GOLDEN)
    assert bad == [], f"{tag}: {len(got)} surfels, fixture {g['final_n']}: {bad}"


def _ff(api, cam, **kw):
    kw.setdefault("flags", api.DSM_FLAG_EIGEN33_PRODUCTS)
    return api.FusionFunctions.from_camera(cam, **kw)


@pytest.mark.parametrize("name", ["tiny_40", "tiny_ragged_40", "kitti1226_24", "vga_rgbd_8"])
def test_dropin_per_frame(mods, gold, name):
    """dsm_fuse_map frame by frame: counts, label image, seed table and map digests after every frame, and the final map"""
    api, synth, ob, E = mods
    case, g = _case(gold, E, name)
    ff = _ff(api, getattr(synth, case["camera"]), surfel_capacity=1 << 20)
    lg = np.zeros(0, api.SURFEL_DTYPE)
    for (t, img, dep, pose, ref), want in zip(E.sequence(case, synth), g["per_frame"]):
        lg, k = ff.fuse_map(ref, img, dep, pose, lg)
        got = E.frame_record(k, lg, ff.labels(), ff.seeds())
        assert got == want, f"{name} frame {t}: " + str({f: (got[f], want[f]) for f in got if got[f] != want[f]})
    _check_final(name, lg, g)
    ff.close()


def _replay(api, ff, frames, splits):
    """all frames resident, enqueued in calls of the given lengths"""
    for t, img, dep, pose, ref in frames:
        ff.frame_upload(t, img, dep)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    i = 0
    for m in splits:
        part = frames[i:i + m]
        ff.replay_enqueue(*ff.pack_replay([f[0] for f in part], [f[4] for f in part], np.stack([f[3] for f in part])))
        i += m
    assert i == len(frames)
    ff.synchronize()
    return ff.map_download()


@pytest.mark.parametrize("depth", [1, 8, 24])
@pytest.mark.parametrize("name", ["tiny_ragged_40", "kitti1226_24"])
def test_replay_enqueue(mods, gold, name, depth):
    """dsm_replay_enqueue at pipeline_depth 1 (one graph per frame), 8 and 24 (frame groups): two calls, the first ending in
    a ragged group"""
    api, synth, ob, E = mods
    case, g = _case(gold, E, name)
    frames = list(E.sequence(case, synth))
    ff = _ff(api, getattr(synth, case["camera"]), frame_slots=len(frames), surfel_capacity=1 << 20, pipeline_depth=depth)
    got = _replay(api, ff, frames, [len(frames) - 13, 13])
    assert len(got) == g["per_frame"][-1]["n_local"]
    _check_final(f"{name} depth {depth}", got, g)
    ff.close()


def test_replay_enqueue_host(mods, gold):
    """dsm_replay_enqueue_host: the frames come with the call, uploaded on the streams of their frame groups"""
    api, synth, ob, E = mods
    case, g = _case(gold, E, "kitti1226_24")
    frames = list(E.sequence(case, synth))
    ff = _ff(api, getattr(synth, case["camera"]), frame_slots=8, surfel_capacity=1 << 20, pipeline_depth=8)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    pin = api.PinnedFrames(ff, len(frames))
    for t, img, dep, pose, ref in frames:
        pin.set(t, img, dep)
    _, refs, poses = ff.pack_replay([f[0] for f in frames], [f[4] for f in frames], np.stack([f[3] for f in frames]))
    ff.replay_enqueue_host(pin, 0, refs[:19], poses[:19])
    ff.replay_enqueue_host(pin, 19, refs[19:], poses[19:])
    ff.replay_wait()
    _check_final("kitti1226_24 host frames", ff.map_download(), g)
    pin.close()
    ff.close()


def test_batch_of_eight(mods, gold):
    """dsm_batch_replay_enqueue over eight handles with the flag: the lane-per-seed kernels"""
    api, synth, ob, E = mods
    case, g = _case(gold, E, "kitti1226_24")
    frames = list(E.sequence(case, synth))
    cam = getattr(synth, case["camera"])
    hs = []
    for b in range(8):
        ff = _ff(api, cam, frame_slots=len(frames), surfel_capacity=1 << 20, pipeline_depth=1)
        for t, img, dep, pose, ref in frames:
            ff.frame_upload(t, img, dep)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        hs.append(ff)
    plan = api.FusionFunctions.pack_replay([f[0] for f in frames], [f[4] for f in frames], np.stack([f[3] for f in frames]))
    batch = api.Batch(hs)
    first = 11
    s, r, p, _ = api.Batch.pack([(plan[0][:first], plan[1][:first], plan[2][:first])] * 8)
    batch.replay_enqueue(s, r, p, first)
    s, r, p, _ = api.Batch.pack([(plan[0][first:], plan[1][first:], plan[2][first:])] * 8)
    batch.replay_enqueue(s, r, p, len(frames) - first)
    batch.synchronize()
    for b, ff in enumerate(hs):
        _check_final(f"batched handle {b}", ff.map_download(), g)
    batch.close()
    for ff in hs:
        ff.close()


def _edge_frames(synth, camera):
    from test_gpu_parity import edge_cases
    return edge_cases(getattr(synth, camera))


@pytest.mark.parametrize("camera", ["TINY_RAGGED", "KITTI_1226"])
def test_edge_cases_dropin(mods, gold, camera):
    """the hostile frames, fused twice each through dsm_fuse_map: every record of both steps, and the final maps"""
    api, synth, ob, E = mods
    g = next(e for e in gold["edge_cases"] if e["camera"] == camera)
    finals = np.load(os.path.join(GOLDEN, g["final_maps"]))
    ff = _ff(api, getattr(synth, camera), surfel_capacity=1 << 20)
    for name, (img, dep) in _edge_frames(synth, camera).items():
        lg = np.zeros(0, api.SURFEL_DTYPE)
        for ridx in (0, 1):
            lg, k = ff.fuse_map(ridx, img, dep, E.EDGE_POSES[ridx], lg)
            assert E.frame_record(k, lg, ff.labels(), ff.seeds()) == g["cases"][name]["steps"][ridx], (camera, name, ridx)
        assert fields_equal(lg, finals[name]) == [], (camera, name)
    ff.close()


def test_edge_cases_batched(mods, gold):
    """the same frames through batches of eight handles at 1226x370 (lane-per-seed kernels), one case per handle"""
    api, synth, ob, E = mods
    camera = "KITTI_1226"
    g = next(e for e in gold["edge_cases"] if e["camera"] == camera)
    finals = np.load(os.path.join(GOLDEN, g["final_maps"]))
    cases = list(_edge_frames(synth, camera).items())
    cam = getattr(synth, camera)
    poses = np.stack(E.EDGE_POSES)
    for lo in range(0, len(cases), 8):
        chunk = (cases[lo:lo + 8] + cases[:8])[:8]  # (the last batch is filled up with cases already seen)
        hs, plans = [], []
        for name, (img, dep) in chunk:
            ff = _ff(api, cam, frame_slots=2, surfel_capacity=1 << 20, pipeline_depth=1)
            ff.frame_upload(0, img, dep)
            ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
            hs.append(ff)
            plans.append(api.FusionFunctions.pack_replay([0, 0], [0, 1], poses))
        batch = api.Batch(hs)
        s, r, p, _ = api.Batch.pack(plans)
        batch.replay_enqueue(s, r, p, 2)
        batch.synchronize()
        for (name, _), ff in zip(chunk, hs):
            got = ff.map_download()
            assert len(got) == g["cases"][name]["steps"][1]["n_local"], name
            assert fields_equal(got, finals[name]) == [], name
        batch.close()
        for ff in hs:
            ff.close()


def test_control_without_the_flag(mods, gold):
    """The same inputs without the flag: the Eigen 3.2 order of the C restatement, byte for byte, and not the fixtures --
    dropped in and replayed in frame groups"""
    api, synth, ob, E = mods
    for name in ("tiny_40", "kitti1226_24"):
        case, g = _case(gold, E, name)
        cam = getattr(synth, case["camera"])
        frames = list(E.sequence(case, synth))
        orc = ob.PortOracle(cam)
        lo = np.zeros(0, ob.SURFEL_DTYPE)
        for t, img, dep, pose, ref in frames:
            lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
        lo = lo.astype(api.SURFEL_DTYPE)
        ff = _ff(api, cam, flags=0, surfel_capacity=1 << 20)
        lg = np.zeros(0, api.SURFEL_DTYPE)
        for t, img, dep, pose, ref in frames:
            lg, _ = ff.fuse_map(ref, img, dep, pose, lg)
        ff.close()
        ff = _ff(api, cam, flags=0, frame_slots=len(frames), surfel_capacity=1 << 20, pipeline_depth=24)
        lr = _replay(api, ff, frames, [len(frames)])
        ff.close()
        for tag, got in (("drop-in", lg), ("replay", lr)):
            assert len(got) == len(lo) and fields_equal(got, lo) == [], (name, tag)
            assert E.final_map_differences(got, g, GOLDEN) != [], (name, tag, "equals the Eigen >= 3.3 fixture")


def test_mixed_flags_batch_is_refused(mods):
    api, synth, ob, E = mods
    cam = synth.TINY
    a = _ff(api, cam, pipeline_depth=1)
    b = _ff(api, cam, flags=0, pipeline_depth=1)
    with pytest.raises(api.DsmError) as e:
        api.Batch([a, b])
    assert e.value.code == api.DSM_E_INVALID
    api.Batch([a, _ff(api, cam, pipeline_depth=1)]).close()  # agreeing handles are fine
    a.close()
    b.close()


def test_node_with_engine_flags(mods, gold):
    """The node with engine_flags = DSM_FLAG_EIGEN33_PRODUCTS against the reference node built with the stand-in: every
    keyframe pose, surfel, inactive point and exported byte; without the flag the same stream ends elsewhere"""
    import node_state
    from densesurfelmapping_amd import surfel_map
    api, synth, ob, E = mods
    g = gold["node"]
    briefs, checkpoints, final, files = E.run_node(
        lambda cam, d: surfel_map.SurfelMap(cam, drift_free_poses=d, engine_flags=api.DSM_FLAG_EIGEN33_PRODUCTS), synth, node_state)
    assert briefs == g["briefs"]
    ref = np.load(os.path.join(GOLDEN, g["final"]))
    for key in ("attached_counts", "begin", "is_local", "links"):
        assert np.array_equal(final[key], ref[key]), key
    assert final["poses"].tobytes() == ref["poses"].tobytes()
    for key in ("local", "attached"):
        assert fields_equal(final[key], ref[key]) == [], key
    a, b = final["cloud"], ref["cloud"]  # (NaN == NaN: the sign of a NaN is not defined by the reference's arithmetic)
    assert a.shape == b.shape and ((a.view("u4") == b.view("u4")) | (np.isnan(a) & np.isnan(b))).all(), "inactive_pointcloud"
    assert checkpoints == g["checkpoints"] and node_state.digest(final) == g["final_digest"]
    assert files == g["files"]
    _, _, final0, _ = E.run_node(lambda cam, d: surfel_map.SurfelMap(cam, drift_free_poses=d), synth, node_state)
    assert node_state.digest(final0) != g["final_digest"]
    with pytest.raises(api.DsmError):  # any other engine bit is refused
        surfel_map.SurfelMap(synth.NODE_CAM, engine_flags=api.DSM_FLAG_NO_GRAPH)


def _raw_expect(image, depth, pose7, fx, fy, cx, cy, eigen33):
    """publish_raw_pointcloud (SM.cpp:1115-1151) in float32, operation by operation; rotation_R * cam_point in Eigen 3.2's
    ((a0 b0 + a1 b1) + a2 b2) or Eigen >= 3.3's (a0 b0 + (a1 b1 + a2 b2)) order (numpy does not contract to FMA)"""
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
            if eigen33:
                out[..., r] = (R[r][0] * c[0] + (R[r][1] * c[1] + R[r][2] * c[2])) + T[r]
            else:
                out[..., r] = ((R[r][0] * c[0] + R[r][1] * c[1]) + R[r][2] * c[2]) + T[r]
    out[..., 3] = image.T.astype(np.float32)
    return out.reshape(-1, 4)


def _bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 4)
    b = np.ascontiguousarray(b, np.float32).reshape(-1, 4)
    return a.shape == b.shape and np.array_equal(a.view("u4"), b.view("u4"))


def test_raw_cloud_follows_the_flag(mods):
    """dsm_frame_cloud with the flag == the Eigen >= 3.3 restatement on adversarial depths and non-unit quaternions, which
    differs from the Eigen 3.2 one; a handle without the flag still gives the 3.2 cloud"""
    from test_gpu_clouds import _adversarial_frame
    api, synth, ob, E = mods
    rng = np.random.default_rng(33)
    fx, fy, cx, cy = 57.25, 55.5, 31.3, 15.7
    moved = 0
    for (w, h) in ((64, 32), (203, 77), (1226, 370)):
        handles = {}
        for e33 in (True, False):
            ff = api.FusionFunctions()
            ff.initialize(w, h, fx, fy, cx, cy, 30.0, 0.3, surfel_capacity=1 << 16, frame_slots=2,
                          flags=api.DSM_FLAG_EIGEN33_PRODUCTS if e33 else 0)
            handles[e33] = ff
        for slot in (0, 1):
            image, depth = _adversarial_frame(rng, w, h)
            q = rng.normal(size=4) * rng.choice([1.0, 0.3, 2.7])  # random, not unit
            pose7 = np.concatenate([rng.normal(size=3) * 10, q])
            e33, e32 = (_raw_expect(image, depth, pose7, fx, fy, cx, cy, v) for v in (True, False))
            moved += int((e33.view("u4") != e32.view("u4")).any(axis=1).sum())
            for flag, ff in handles.items():
                ff.frame_upload(slot, image, depth)
                assert _bits_equal(ff.frame_cloud(slot, pose7), e33 if flag else e32), (w, h, slot, flag)
        for ff in handles.values():
            ff.close()
    assert moved > 0


def test_node_raw_publication_follows_the_flag(mods):
    """The node's RAW cloud, published after every fuse, with engine_flags = DSM_FLAG_EIGEN33_PRODUCTS: the Eigen >= 3.3
    restatement of the fused frame under the fuse pose"""
    import node_state
    from densesurfelmapping_amd import surfel_map
    api, synth, ob, E = mods
    case = next(c for c in node_state.SCENARIOS if c["name"] == E.NODE_SCENARIO)
    cam, scene = node_state.camera_and_scene(case, synth)
    node = surfel_map.SurfelMap(cam, drift_free_poses=case["drift_free_poses"], engine_flags=api.DSM_FLAG_EIGEN33_PRODUCTS)
    frames, problems, n_pub = {}, [], [0, 0]

    def on_publish(pub):
        try:
            image, depth = frames[pub["stamp"]]
            want = _raw_expect(image, depth, pub["fuse_pose"], cam.fx, cam.fy, cam.cx, cam.cy, True)
            assert _bits_equal(pub["clouds"]["raw"], want), len(problems)
            n_pub[1] += not _bits_equal(want, _raw_expect(image, depth, pub["fuse_pose"], cam.fx, cam.fy, cam.cx, cam.cy, False))
        except Exception as e:  # (exceptions do not cross the C callback: collect them)
            problems.append(repr(e))
        n_pub[0] += 1

    node.set_publish(("raw",), on_publish)
    kw = dict(case["kw"])
    kw["frames"] = {tl: synth.render(cam, scene, tl)[:2] for tl in range(kw["lap"])}
    for ev in synth.node_messages(cam, E._TiltedScene(scene), 20, **kw):
        if ev[0] in ("image", "depth"):
            f = frames.setdefault(tuple(ev[1]), [None, None])
            f[0 if ev[0] == "image" else 1] = np.array(ev[2])
        node.feed(ev)
    node.close()
    assert problems == [], problems[:3]
    assert n_pub[0] >= 15 and n_pub[1] > 0, n_pub
