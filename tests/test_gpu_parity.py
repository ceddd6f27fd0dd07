"""GPU parity: the HIP path, called through the C ABI, against the CPU oracle on identical inputs.

Bar (BASELINE.json north_star): superpixel label image and surfel count bit-exact, float attributes
within 1e-4 relative.  The HIP path reproduces the reference's operation order, so these tests hold it
to the stricter bar first -- every byte equal, NaN == NaN -- and state the 1e-4 tolerance as the
fallback contract in `fields_close`.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import ROOT, fields_close, fields_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(oracle_built):
    import torch
    torch.cuda.init()  # torch's lazy HIP initialisation first: tests below hand torch device memory to the library
    from densesurfelmapping_amd import api, synth
    from oracle import bindings
    return api, synth, bindings


def _compare_frame(tag, ff, orc, loc_g, loc_o):
    lab_g, lab_o = ff.labels(), orc.labels()
    n_bad = int((lab_g != lab_o).sum())
    assert n_bad == 0, f"{tag}: {n_bad} label mismatches, first at {np.argwhere(lab_g != lab_o)[:5].tolist()}"
    sg, so = ff.seeds(), orc.seeds()
    bad = fields_equal(sg, so)
    assert not bad, f"{tag}: seed table differs {bad}"
    assert len(loc_g) == len(loc_o), f"{tag}: surfel count {len(loc_g)} vs {len(loc_o)}"
    bad = fields_equal(loc_g, loc_o)
    assert not bad, f"{tag}: surfels differ {bad}"
    fields_close(loc_g, loc_o, rtol=1e-4)


@pytest.mark.parametrize("flags", [1, 0], ids=["eager", "graph"])
def test_dropin_fuse_map_tiny_sequence(mods, flags):
    """SurfelMap::fuse_map drop-in, host buffers in/out, 60 frames (prune + compaction reached)."""
    api, synth, ob = mods
    cam, scene = synth.TINY, synth.Scene()
    ff = api.FusionFunctions.from_camera(cam, flags=flags, surfel_capacity=65536)
    orc = ob.PortOracle(cam)
    lg = np.zeros(0, api.SURFEL_DTYPE)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for t, img, dep, pose, ref in synth.sequence(cam, scene, 60):
        lg, kg = ff.fuse_map(ref, img, dep, pose, lg)
        lo, ko = orc.fuse_map(ref, img, dep, pose, lo)
        assert kg == ko, f"frame {t}: new surfel count {kg} vs {ko}"
        _compare_frame(f"frame {t}", ff, orc, lg, lo.astype(api.SURFEL_DTYPE))


def test_dropin_fuse_initialize_map(mods):
    """FusionFunctions::fuse_initialize_map drop-in: local updated in place, new surfels separate."""
    api, synth, ob = mods
    cam, scene = synth.TINY, synth.Scene(seed=7)
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=65536)
    orc = ob.PortOracle(cam)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for t, img, dep, pose, ref in synth.sequence(cam, scene, 12):
        g_local, g_new = ff.fuse_initialize_map(ref, img, dep, pose, lo)
        o_local, o_new = orc.fuse_initialize_map(ref, img, dep, pose, lo)
        assert not fields_equal(g_local, o_local.astype(api.SURFEL_DTYPE)), f"frame {t} local"
        assert not fields_equal(g_new, o_new.astype(api.SURFEL_DTYPE)), f"frame {t} new"
        lo, _ = orc.fuse_map(ref, img, dep, pose, lo)


def test_dropin_shadow_detects_caller_edits(mods):
    """dsm_fuse_map keeps a page-locked shadow of what it returned and skips the map upload when the caller hands the
    same bytes back.  Everything that can make the device map differ from the caller's array must be noticed: edits of
    single records, a shorter or longer array, resident calls in between, fuse_initialize_map in between."""
    api, synth, ob = mods
    cam, scene = synth.VGA_DRIVE, synth.Scene(seed=41)
    ff = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=1 << 18)
    orc = ob.PortOracle(cam)
    buf = np.zeros(1 << 17, api.SURFEL_DTYPE)
    n = 0
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    rng = np.random.default_rng(2)
    for t, img, dep, pose, ref in synth.sequence(cam, scene, 16):
        if t == 3:      # one record edited in place (same length)
            buf["pz"][n // 2] += 0.25
            lo["pz"][n // 2] += 0.25
        if t == 5:      # records deleted by the caller (move_add_surfels marks update_times = 0, SM.cpp:1494)
            kill = rng.random(n) < 0.2
            buf["update_times"][:n][kill] = 0
            lo["update_times"][kill] = 0
        if t == 7:      # shorter array
            n -= 100
            lo = lo[:n].copy()
        if t == 9:      # longer array: surfels of a re-activated keyframe appended (SM.cpp:1583-1590)
            extra = lo[:50].copy()
            extra["px"] += 0.5
            buf[n:n + 50] = extra.astype(api.SURFEL_DTYPE)
            lo = np.concatenate([lo, extra])
            n += 50
        if t == 11:     # a resident call replaces the device map behind the shadow's back
            ff.map_upload(np.zeros(10, api.SURFEL_DTYPE))
        if t == 13:     # fuse_initialize_map (no compaction) in between: the shadow follows
            g_local, g_new = ff.fuse_initialize_map(ref, img, dep, pose, buf[:n])
            o_local, o_new = orc.fuse_initialize_map(ref, img, dep, pose, lo)
            assert fields_equal(g_local, o_local.astype(api.SURFEL_DTYPE)) == [] and fields_equal(g_new, o_new.astype(api.SURFEL_DTYPE)) == []
        n, k = ff.fuse_map_inplace(ref, img, dep, pose, buf, n)
        lo, ko = orc.fuse_map(ref, img, dep, pose, lo)
        assert k == ko and n == len(lo), f"frame {t}"
        assert fields_equal(buf[:n], lo.astype(api.SURFEL_DTYPE)) == [], f"frame {t}"
    ff.close()


def test_dropin_delta_download(mods):
    """The drop-in calls bring back only what a frame changed of the map (round 6: the 64-record groups k_fuse_surfels and
    k_frame_tail flag, packed on the device, one transfer, patched into the shadow and the caller's array; SM.cpp:1066-1073
    hands the same vector to every frame).  90 frames at 1226x370 on the caller's own array, the map growing to 60 k surfels
    with pruning and both compaction branches on the way: after EVERY call the caller's array is the oracle's, byte for byte;
    most calls take the delta path and bring back a fraction of the map.  Then the same through the reference node's own entry
    point (dsm_fuse_initialize_map: no compaction, the caller's loop refills and appends -- SM.cpp:1077-1109 -- so every call sees
    an edited array), and with resident frames in between, which leave flags of their own behind."""
    api, synth, ob = mods
    cam, scene = synth.KITTI_1226, synth.Scene(seed=3)
    frames = list(synth.sequence(cam, scene, 90))
    ff = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=1 << 18)
    orc = ob.PortOracle(cam)
    buf = np.zeros(1 << 17, api.SURFEL_DTYPE)
    n, lo = 0, np.zeros(0, ob.SURFEL_DTYPE)
    shrank = grew = False
    for t, img, dep, pose, ref in frames:
        before = n
        n, k = ff.fuse_map_inplace(ref, img, dep, pose, buf, n)
        lo, ko = orc.fuse_map(ref, img, dep, pose, lo)
        assert k == ko and n == len(lo), f"frame {t}"
        assert fields_equal(buf[:n], lo.astype(api.SURFEL_DTYPE)) == [], f"frame {t}"
        shrank |= n < before
        grew |= n > before
        if t == 40:  # resident frames in between: the map moves on behind the shadow's back, their flags stay behind
            ff.frame_upload(0, frames[41][1], frames[41][2])
            ff.fuse_frame_resident(0, frames[41][4], frames[41][3])
            ff.synchronize()
            ff.map_upload(buf[:n])  # (back to the caller's state: the flags the resident frame set are stale now)
    st = ff.debug_dropin_stats()
    assert st["calls"] == 90 and st["delta_calls"] >= 60, st
    groups_in_map = (n + 63) // 64
    assert st["delta_groups"] / st["delta_calls"] < 0.6 * groups_in_map, (st, groups_in_map)
    assert grew and shrank and n > 40000
    print("drop-in delta download:", st, "groups in the final map:", groups_in_map)
    ff.close()
    # ---- the reference node's own path: fuse_initialize_map + the caller's compaction loop (here: the oracle's fuse_map, which
    # IS that loop) -- the array the next call sees was edited by the caller every time
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 18)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for t, img, dep, pose, ref in frames[:40]:
        g_local, g_new = ff.fuse_initialize_map(ref, img, dep, pose, lo)
        o_local, o_new = orc.fuse_initialize_map(ref, img, dep, pose, lo)
        assert fields_equal(g_local, o_local.astype(api.SURFEL_DTYPE)) == [], f"frame {t}: local"
        assert fields_equal(g_new, o_new.astype(api.SURFEL_DTYPE)) == [], f"frame {t}: new"
        lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
    st = ff.debug_dropin_stats()
    assert st["calls"] == 40 and st["delta_calls"] >= 20, st
    ff.close()


def test_resident_replay_kitti(mods):
    """BASELINE config 2 shape: 1226x370, map and frames resident in HBM, one graph replay per frame."""
    api, synth, ob = mods
    cam, scene = synth.KITTI_1226, synth.Scene()
    n = 16
    ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=1 << 20)
    orc = ob.PortOracle(cam)
    frames = list(synth.sequence(cam, scene, n))
    for t, img, dep, pose, ref in frames:
        ff.frame_upload(t, img, dep)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for t, img, dep, pose, ref in frames:
        ff.fuse_frame_resident(t, ref, pose)
        lo, ko = orc.fuse_map(ref, img, dep, pose, lo)
        assert ff.last_new_count() == ko
        _compare_frame(f"kitti frame {t}", ff, orc, ff.map_download(), lo.astype(api.SURFEL_DTYPE))


def test_parity_sequence_200_frames(mods):
    """the 200-frame parity sequence (four scene periods: the map saturates, stale surfels are pruned,
    holes are refilled and compacted), replayed resident in one enqueue with frame pipelining; checkpoints every 50
    frames against the oracle, byte for byte."""
    api, synth, ob = mods
    cam, scene = synth.TINY, synth.Scene()
    period = scene.frames_per_period
    ff = api.FusionFunctions.from_camera(cam, frame_slots=period, surfel_capacity=1 << 18)
    orc = ob.PortOracle(cam)
    frames = list(synth.sequence(cam, scene, 200))
    for t in range(period):
        ff.frame_upload(t, frames[t][1], frames[t][2])
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for base in range(0, 200, 50):
        chunk = frames[base:base + 50]
        ff.replay_enqueue(*ff.pack_replay([f[0] % period for f in chunk], [f[4] for f in chunk], [f[3] for f in chunk]))
        for t, img, dep, pose, ref in chunk:
            lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
        got = ff.map_download()
        assert len(got) == len(lo), (base, len(got), len(lo))
        assert fields_equal(got, lo.astype(api.SURFEL_DTYPE)) == [], base
    assert (lo["update_times"] >= 5).sum() > 100
    ff.close()


@pytest.mark.parametrize("camera,frames", [("KITTI_1241", 4), ("FULLHD", 2), ("KITTI_1242", 4), ("TINY_RAGGED", 40)])
def test_other_baseline_sizes(mods, camera, frames):
    """The launch-file default 1241x376 (ragged: 1241 = 155*8 + 1) and BASELINE config 5's 1920x1080, against
    the oracle frame by frame; and sizes with (size mod 8) > 4 -- KITTI raw 1242x375 -- whose last columns / rows
    have no candidate superpixel: label -1 there, as the reference TU also produces in this build (its accesses to
    superpixel_seeds[-1] are undefined behaviour, so parity for those pixels is against the oracle's stated policy)."""
    api, synth, ob = mods
    cam, scene = getattr(synth, camera), synth.Scene(seed=77)
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 20)
    orc = ob.PortOracle(cam)
    lg = np.zeros(0, api.SURFEL_DTYPE)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for t, img, dep, pose, ref in synth.sequence(cam, scene, frames):
        lg, kg = ff.fuse_map(ref, img, dep, pose, lg)
        lo, ko = orc.fuse_map(ref, img, dep, pose, lo)
        assert kg == ko
        _compare_frame(f"{camera} frame {t}", ff, orc, lg, lo.astype(api.SURFEL_DTYPE))
    if cam.width % 8 > 4 or cam.height % 8 > 4:
        lab = ff.labels()
        gw, gh = cam.width // 8, cam.height // 8
        border = np.zeros_like(lab, bool)
        border[:, gw * 8 + 4:] = True
        border[gh * 8 + 4:, :] = True
        assert border.any() and (lab[border] == -1).all() and (lab[~border] >= 0).all()


@pytest.mark.parametrize("camera", ["KITTI_1241", "KITTI_1242"])
def test_launch_default_sizes_through_pruning(mods, camera):
    """The launch files' own image sizes (kitti_orb.launch: 1241x376; KITTI raw 1242x375, whose last columns have no candidate
    superpixel) for longer than the four frames of test_other_baseline_sizes: 60 frames over a 15-frame loop, so that surfels
    are revisited, pruned (FF.cpp:207-211) and refilled / compacted (SM.cpp:1087-1109) at these ragged sizes too -- frame by
    frame (one graph replay each) and again as one pipelined replay with eight frames per batched launch, against the oracle."""
    api, synth, ob = mods
    cam, scene = getattr(synth, camera), synth.Scene(seed=78, frames_per_period=15)
    period, n = scene.frames_per_period, 60
    frames = list(synth.sequence(cam, scene, n))
    orc = ob.PortOracle(cam)
    lo, want, holes = np.zeros(0, ob.SURFEL_DTYPE), [], 0
    for t, img, dep, pose, ref in frames:
        before = len(lo)
        lo, ko = orc.fuse_map(ref, img, dep, pose, lo)
        holes += before + ko - len(lo)
        want.append((ko, len(lo), lo.copy() if (t + 1) % 20 == 0 else None))
    assert holes > 500, "nothing was pruned: the case lost its point"
    ff = api.FusionFunctions.from_camera(cam, frame_slots=period, surfel_capacity=1 << 20)
    for t in range(period):
        ff.frame_upload(t, frames[t][1], frames[t][2])
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    for (t, img, dep, pose, ref), (ko, n_lo, snap) in zip(frames, want):
        ff.fuse_frame_resident(t % period, ref, pose)
        assert (ff.last_new_count(), ff.map_size()) == (ko, n_lo), f"{camera} frame {t}"
        if snap is not None:
            assert fields_equal(ff.map_download(), snap.astype(api.SURFEL_DTYPE)) == [], f"{camera}: map after frame {t}"
    ff.close()
    ff = api.FusionFunctions.from_camera(cam, frame_slots=period, surfel_capacity=1 << 20, pipeline_depth=24)
    for t in range(period):
        ff.frame_upload(t, frames[t][1], frames[t][2])
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    ff.replay_enqueue(*ff.pack_replay([f[0] % period for f in frames], [f[4] for f in frames], [f[3] for f in frames]))
    assert fields_equal(ff.map_download(), lo.astype(api.SURFEL_DTYPE)) == [], f"{camera}: pipelined replay"
    ff.close()


def test_api_errors_are_reported(mods):
    """The reference returns void and prints; the ABI returns a status and a message, and never computes on bad input."""
    api, synth, ob = mods
    cam = synth.TINY
    with pytest.raises(api.DsmError) as ei:  # fewer than 3x3 superpixel cells
        api.FusionFunctions().initialize(20, 96, 100, 100, 80, 48, 30, 0.5)
    assert ei.value.code == -1
    with pytest.raises(api.DsmError) as ei:  # 3840x2160: 129 600 superpixels do not fit the 16-bit label planes
        api.FusionFunctions().initialize(3840, 2160, 2000, 2000, 1920, 1080, 30, 0.5)
    assert ei.value.code == -1 and "65535 superpixels" in str(ei.value)
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=128, frame_slots=2)
    img, dep, pose = synth.render(cam, synth.Scene(), 0)
    with pytest.raises(api.DsmError) as ei:  # resident call before a map exists
        ff.fuse_frame_resident(0, 0, pose)
    assert ei.value.code == -5
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    with pytest.raises(api.DsmError) as ei:  # slot out of range
        ff.frame_upload(2, img, dep)
    assert ei.value.code == -1
    with pytest.raises(api.DsmError) as ei:  # more surfels than the handle can hold
        ff.map_upload(np.zeros(1000, api.SURFEL_DTYPE))
    assert ei.value.code == -4
    with pytest.raises(ValueError):
        ff.fuse_map(0, img[:, :-1], dep, pose, np.zeros(0, api.SURFEL_DTYPE))
    # the asynchronous uploads (ABI 3): slot ranges and frame steps are checked before anything is enqueued
    pin = api.PinnedFrames(ff, 3)
    assert pin.pitch == ff.frame_pitch() and pin.pitch % 64 == 0 and pin.pitch >= cam.width
    for i in range(3):
        pin.set(i, img, dep)
    with pytest.raises(api.DsmError) as ei:  # three frames into two slots
        ff.frames_upload_async(0, pin, 0, 3)
    assert ei.value.code == -1
    with pytest.raises(api.DsmError) as ei:
        ff.frame_upload_async(2, pin.image(0), pin.depth(0))
    assert ei.value.code == -1
    ff.frames_upload_async(0, pin, 1, 2)  # a legal one: both slots, one transfer per plane
    ff.frame_uploads_wait()
    ff.fuse_frame_resident(1, 0, pose)
    ff.synchronize()
    want, _ = ob.PortOracle(cam).fuse_map(0, img, dep, pose, np.zeros(0, ob.SURFEL_DTYPE))
    assert not fields_equal(ff.map_download(), want.astype(api.SURFEL_DTYPE))
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    pin.close()
    with pytest.raises(api.DsmError) as ei:  # an injected label image must hold superpixel indices (it is used as an index)
        ff.debug_set_labels(0, np.full((cam.height, cam.width), ff.n_seed, np.int32))
    assert ei.value.code == -1
    # capacity overflow while appending new surfels is reported, not silently truncated
    ff.frame_upload(0, img, dep)
    nearly_full = np.zeros(120, api.SURFEL_DTYPE)  # live surfels far behind the camera: never touched, never holes
    nearly_full["pz"] = -50.0
    nearly_full["update_times"] = 9
    ff.map_upload(nearly_full)
    ff.fuse_frame_resident(0, 0, pose)  # ~30 new surfels do not fit into the remaining 8 slots
    with pytest.raises(api.DsmError) as ei:
        ff.synchronize()
    assert ei.value.code == -4


def test_quiet_scene_many_stable_seeds(mods):
    """Low-noise, flat-albedo scene: most superpixels stop moving after the first sweep, so most pixels sit
    between stable seeds -- the regime where the scan-order rule (worklist fixed point) decides the labels."""
    api, synth, ob = mods
    cam = synth.VGA_DRIVE
    scene = synth.Scene(seed=3, intensity_noise=1.0, checker=4.0, depth_noise=0.0002, hole_fraction=0.002)
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 20)
    orc = ob.PortOracle(cam)
    lg = np.zeros(0, api.SURFEL_DTYPE)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    stable_seen = 0
    for t, img, dep, pose, ref in synth.sequence(cam, scene, 6):
        lg, kg = ff.fuse_map(ref, img, dep, pose, lg)
        lo, ko = orc.fuse_map(ref, img, dep, pose, lo)
        assert kg == ko
        _compare_frame(f"quiet frame {t}", ff, orc, lg, lo.astype(api.SURFEL_DTYPE))
        stable_seen = max(stable_seen, int(orc.seeds()["stable"].sum()))
    assert stable_seen > ff.n_seed // 3, "the scene no longer produces many stable seeds"


def test_batched_replay_matches_stepwise(mods):
    """dsm_replay_enqueue of a whole subsequence (no host sync in between) == frame-by-frame."""
    api, synth, ob = mods
    cam, scene = synth.VGA_DRIVE, synth.Scene(seed=99)
    n = 24
    ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=1 << 20)
    orc = ob.PortOracle(cam)
    frames = list(synth.sequence(cam, scene, n))
    for t, img, dep, pose, ref in frames:
        ff.frame_upload(t, img, dep)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    slots, refs, poses = api.FusionFunctions.pack_replay([f[0] for f in frames], [f[4] for f in frames],
                                                         np.stack([f[3] for f in frames]))
    ff.replay_enqueue(slots, refs, poses)
    ff.synchronize()
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for t, img, dep, pose, ref in frames:
        lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
    _compare_frame("after 24 frames", ff, orc, ff.map_download(), lo.astype(api.SURFEL_DTYPE))


@pytest.mark.parametrize("fit_small_cap,B", [(None, 5), (None, 8), (40, 9), (0, 5)])
def test_batched_lockstep_replay(mods, fit_small_cap, B):
    """dsm_batch_*: five handles with five different scenes advance in lockstep, every kernel launched once for all of
    them (grid z = handle); each subsequence's map equals the oracle's for its own scene, and a handle used alone
    afterwards continues correctly.  Batched launches fit the seed planes in two tiers (short LDS columns for nearly
    all groups of seeds, a queue worked off by a full-length kernel for the rest); these scenes never fill the queue,
    so the runs with a lowered limit send most (40) or all (0) groups through it."""
    api, synth, ob = mods
    # (batches of fewer than eight handles launch the per-seed stages with a wave per seed, from eight on with a lane per
    # seed and four pixels per thread in the assignment: both forms are exercised)
    cam = synth.VGA_DRIVE
    n = 14
    scenes = [synth.Scene(seed=200 + 7 * b, n_boxes=6 + b) for b in range(B)]
    handles, plans, frames = [], [], []
    for b in range(B):
        ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=1 << 18, pipeline_depth=1)
        if fit_small_cap is not None:
            ff.debug_set_fit_small_cap(fit_small_cap)
        fr = list(synth.sequence(cam, scenes[b], n))
        for t, img, dep, pose, ref in fr:
            ff.frame_upload(t, img, dep)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        plans.append(api.FusionFunctions.pack_replay([f[0] for f in fr], [f[4] for f in fr], np.stack([f[3] for f in fr])))
        handles.append(ff)
        frames.append(fr)
    batch = api.Batch(handles)
    first = 9
    s, r, p, _ = api.Batch.pack([(pl[0][:first], pl[1][:first], pl[2][:first]) for pl in plans])
    batch.replay_enqueue(s, r, p, first)
    s, r, p, _ = api.Batch.pack([(pl[0][first:n - 1], pl[1][first:n - 1], pl[2][first:n - 1]) for pl in plans])
    batch.replay_enqueue(s, r, p, n - 1 - first)
    batch.synchronize()
    for b in range(B):
        orc = ob.PortOracle(cam)
        lo = np.zeros(0, ob.SURFEL_DTYPE)
        for t, img, dep, pose, ref in frames[b][:n - 1]:
            lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
        _compare_frame(f"batched subsequence {b}", handles[b], orc, handles[b].map_download(), lo.astype(api.SURFEL_DTYPE))
        # the handle on its own again: the last frame through its own stream
        t, img, dep, pose, ref = frames[b][n - 1]
        handles[b].fuse_frame_resident(t, ref, pose)
        lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
        _compare_frame(f"subsequence {b} alone after the batch", handles[b], orc, handles[b].map_download(), lo.astype(api.SURFEL_DTYPE))
    with pytest.raises(api.DsmError):  # handles whose parameter rings are out of step cannot be batched
        api.Batch([handles[0], api.FusionFunctions.from_camera(cam, pipeline_depth=1)])
    batch.close()
    for ff in handles:
        ff.close()


def test_caller_provided_pose_inverse(mods):
    """DSM_ABI_VERSION 3, the *_inv entry points (include/dsm.h): the reference inverts the pose with the caller's Eigen
    (FF.cpp:59); fed the inverses "another Eigen build" produced -- tests/golden/inv_pose_perturbed.npz, recorded from the
    reference's own TU with every element of Matrix4f::inverse() moved by up to two ulps (make_golden_inv.py) -- the
    engine reproduces THAT build's map byte for byte, through the drop-in call and through the resident replay; without
    them it reproduces the unperturbed one, which differs."""
    api, synth, ob = mods
    g = np.load(os.path.join(ROOT, "tests", "golden", "inv_pose_perturbed.npz"))
    cam, scene, n = getattr(synth, str(g["camera"])), synth.Scene(seed=int(g["scene_seed"])), int(g["frames"])
    want = g["final_map"].astype(api.SURFEL_DTYPE)
    frames = list(synth.sequence(cam, scene, n))
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=65536)
    lg = np.zeros(0, api.SURFEL_DTYPE)
    for t, img, dep, pose, ref in frames:
        lg, k = ff.fuse_map(ref, img, dep, pose, lg, inv_pose=g["inv_poses_cm"][t])
        assert (k, len(lg)) == (int(g["n_new"][t]), int(g["n_local"][t])), f"frame {t}"
    assert not fields_equal(lg, want), "drop-in with the caller's inverses"
    ff.close()
    # the resident replay with the same inverses
    ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=65536)
    for t, img, dep, pose, ref in frames:
        ff.frame_upload(t, img, dep)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    s, r, p = api.FusionFunctions.pack_replay([f[0] for f in frames], [f[4] for f in frames], np.stack([f[3] for f in frames]))
    ff.replay_enqueue(s[:n - 1], r[:n - 1], p[:n - 1], inv_poses_cm=g["inv_poses_cm"][:n - 1])
    ff.fuse_frame_resident(n - 1, frames[-1][4], frames[-1][3], inv_pose=g["inv_poses_cm"][n - 1])
    ff.synchronize()
    assert not fields_equal(ff.map_download(), want), "resident replay with the caller's inverses"
    ff.close()
    # control: the library's own closed form gives the UNperturbed TU's map, which is another one
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=65536)
    lg = np.zeros(0, api.SURFEL_DTYPE)
    for t, img, dep, pose, ref in frames:
        lg, _ = ff.fuse_map(ref, img, dep, pose, lg)
    assert len(lg) != len(want) or fields_equal(lg, want), "the perturbation pattern of the golden must matter"
    ff.close()


def test_handles_and_batches_driven_from_threads(mods):
    """The device's four per-queue streams are shared by every batch and every frame-group lead of the process; graphs are
    captured on private streams, so threads driving different handles / batches never see each other's captures
    (ADVICE r03): two pipelined handles (depth 4: frame groups on the shared streams) on a thread each, then eight
    batches of two handles with a thread each -- more batches than reserved streams, all capturing their graphs at
    their first frame at the same time.  Every map equals the same replay done on one thread."""
    import threading
    api, synth, ob = mods
    cam, n = synth.TINY, 24
    scenes = [synth.Scene(seed=400 + 3 * b) for b in range(16)]
    seqs = [list(synth.sequence(cam, sc, n)) for sc in scenes]

    def make(b, depth):
        ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=65536, pipeline_depth=depth)
        for t, img, dep, pose, ref in seqs[b]:
            ff.frame_upload(t, img, dep)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        return ff

    def plan(b):
        fr = seqs[b]
        return api.FusionFunctions.pack_replay([f[0] for f in fr], [f[4] for f in fr], np.stack([f[3] for f in fr]))

    want = []
    for b in range(16):  # one thread, one handle at a time
        ff = make(b, 1)
        ff.replay_enqueue(*plan(b))
        ff.synchronize()
        want.append(ff.map_download())
        ff.close()
    errors = []

    def guarded(fn, *a):
        try:
            fn(*a)
        except Exception as e:  # noqa: BLE001 -- reported below, in the main thread
            errors.append(repr(e))

    # two pipelined handles, a thread each
    hs = [make(b, 4) for b in range(2)]
    def drive_handle(b):
        s, r, p = plan(b)
        for lo in range(0, n, 8):  # several enqueue calls: first capture, then replays
            hs[b].replay_enqueue(s[lo:lo + 8], r[lo:lo + 8], p[lo:lo + 8])
        hs[b].synchronize()
    th = [threading.Thread(target=guarded, args=(drive_handle, b)) for b in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    for b in range(2):
        assert not fields_equal(hs[b].map_download(), want[b]), f"pipelined handle {b} driven from its own thread"
        hs[b].close()
    # eight batches of two handles, a thread each
    hs = [make(b, 1) for b in range(16)]
    batches = [api.Batch(hs[2 * k:2 * k + 2]) for k in range(8)]
    def drive_batch(k):
        s, r, p, _ = api.Batch.pack([plan(2 * k), plan(2 * k + 1)])
        s, r, p = s.reshape(2, n), r.reshape(2, n), p.reshape(2, n, 16)
        for lo in range(0, n, 6):
            batches[k].replay_enqueue(np.ascontiguousarray(s[:, lo:lo + 6]).ravel(), np.ascontiguousarray(r[:, lo:lo + 6]).ravel(),
                                      np.ascontiguousarray(p[:, lo:lo + 6]).reshape(-1, 16), 6)
        batches[k].synchronize()
    th = [threading.Thread(target=guarded, args=(drive_batch, k)) for k in range(8)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    for b in range(16):
        assert not fields_equal(hs[b].map_download(), want[b]), f"handle {b} of batch {b // 2}, one thread per batch"
    for bt in batches:
        bt.close()
    for ff in hs:
        ff.close()


def test_rgbd_constant_set(mods):
    """BASELINE config 4 shape: 640x480 with the RGB-D constants of fusion_functions.h:17-21."""
    api, synth, ob = mods
    cam, scene = synth.VGA_RGBD, synth.Scene(scale=0.12, step=0.05, seed=5)
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 20)
    orc = ob.PortOracle(cam)
    lg = np.zeros(0, api.SURFEL_DTYPE)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for t, img, dep, pose, ref in synth.sequence(cam, scene, 8):
        lg, kg = ff.fuse_map(ref, img, dep, pose, lg)
        lo, ko = orc.fuse_map(ref, img, dep, pose, lo)
        assert kg == ko
        _compare_frame(f"rgbd frame {t}", ff, orc, lg, lo.astype(api.SURFEL_DTYPE))


def edge_cases(cam):
    """{name: (image, depth)}: the hostile frames of test_edge_inputs at any camera size (also fed to the batched kernels,
    tests/test_gpu_adversarial.py)."""
    rng = np.random.default_rng(3)
    cases = {
        "zero depth": (np.full((cam.height, cam.width), 100, np.uint8), np.zeros((cam.height, cam.width), np.float32)),
        "flat wall": (np.full((cam.height, cam.width), 128, np.uint8), np.full((cam.height, cam.width), 4.0, np.float32)),
        # depth stays in the sensor's range: values in (0.01, ~0.05) m make every candidate cost exceed
        # the reference's 1e6 sentinel, after which it indexes superpixel_seeds[-1] (FF.cpp:442-451)
        "noise": (rng.integers(0, 256, (cam.height, cam.width)).astype(np.uint8),
                  np.where(rng.random((cam.height, cam.width)) < 0.15, 0.0,
                           rng.uniform(0.4, 8.0, (cam.height, cam.width))).astype(np.float32)),
    }
    half = cases["flat wall"][1].copy()
    half[::2] = 0.0
    cases["striped holes"] = (cases["noise"][0], half)
    # what a publisher can hand over besides metres (kitti_publisher/scripts/publisher.py:38 divides by the disparity: +inf
    # where it is 0): non-finite and negative depths, alone and mixed into ordinary ones
    nd = cases["noise"][1]
    u = rng.random(nd.shape)
    cases["inf sky"] = (cases["noise"][0], np.where(np.arange(cam.height)[:, None] < cam.height // 3, np.float32(np.inf), cases["flat wall"][1]).astype(np.float32))
    cases["all inf"] = (cases["flat wall"][0], np.full(nd.shape, np.inf, np.float32))
    cases["inf speckle"] = (cases["noise"][0], np.where(u < 0.1, np.float32(np.inf), nd).astype(np.float32))
    cases["nan speckle"] = (cases["noise"][0], np.where(u < 0.1, np.float32(np.nan), nd).astype(np.float32))
    cases["negative speckle"] = (cases["noise"][0], np.where(u < 0.1, -nd - 1.0, nd).astype(np.float32))
    cases["everything"] = (cases["noise"][0], np.where(u < 0.05, np.float32(np.inf), np.where(u < 0.1, np.float32(np.nan),
                                                       np.where(u < 0.15, np.float32(-np.inf), np.where(u < 0.2, -nd, nd)))).astype(np.float32))
    # few grey levels over a flat wall: whole regions of exact cost ties (the first candidate in scan order wins, FF.cpp:430)
    cases["two greys"] = (np.where((np.arange(cam.width)[None, :] // 24 + np.arange(cam.height)[:, None] // 16) % 2, 64, 192).astype(np.uint8), cases["flat wall"][1])
    return cases


def test_edge_inputs(mods):
    """Empty depth (no surfels), all-holes rows, constant image: same answers as the oracle."""
    api, synth, ob = mods
    cam = synth.TINY
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=65536)
    orc = ob.PortOracle(cam)
    pose = np.eye(4, dtype=np.float32)
    for name, (img, dep) in edge_cases(cam).items():
        lg, kg = ff.fuse_map(0, img, dep, pose, np.zeros(0, api.SURFEL_DTYPE))
        lo, ko = orc.fuse_map(0, img, dep, pose, np.zeros(0, ob.SURFEL_DTYPE))
        assert kg == ko, name
        _compare_frame(name, ff, orc, lg, lo.astype(api.SURFEL_DTYPE))
        # second pass over the map just created (fusion branch)
        lg, kg = ff.fuse_map(1, img, dep, pose, lg)
        lo, ko = orc.fuse_map(1, img, dep, pose, lo)
        _compare_frame(name + " (2nd)", ff, orc, lg, lo.astype(api.SURFEL_DTYPE))


def test_strided_rows_like_a_cv_mat_roi(mods):
    """image / depth rows with a step larger than the row (a cv::Mat ROI): the pitched 2-D copy path gives the
    same frame as the tightly packed fast path (1-D copy + device repack)."""
    api, synth, ob = mods
    cam, scene = synth.TINY, synth.Scene()
    ff_a = api.FusionFunctions.from_camera(cam, surfel_capacity=65536)
    ff_b = api.FusionFunctions.from_camera(cam, surfel_capacity=65536)
    la = lb = np.zeros(0, api.SURFEL_DTYPE)
    for t, img, dep, pose, ref in synth.sequence(cam, scene, 6):
        wide_i = np.zeros((cam.height, cam.width + 24), np.uint8)
        wide_d = np.full((cam.height, cam.width + 7), 3.0, np.float32)
        wide_i[:, :cam.width] = img
        wide_d[:, :cam.width] = dep
        vi, vd = wide_i[:, :cam.width], wide_d[:, :cam.width]
        assert vi.strides[0] != cam.width and vd.strides[0] != cam.width * 4
        la, ka = ff_a.fuse_map(ref, img, dep, pose, la)
        lb, kb = ff_b.fuse_map(ref, vi, vd, pose, lb)
        assert ka == kb and np.array_equal(ff_a.labels(), ff_b.labels())
        assert fields_equal(la, lb) == []
    ff_a.close()
    ff_b.close()


def test_frame_upload_device_and_slot_reuse(mods):
    """dsm_frame_upload_device from torch tensors == host upload; and uploads into a slot whose previous frame is
    still in flight wait for it (two alternating slots, nothing synchronised in between)."""
    import torch
    api, synth, ob = mods
    cam, scene = synth.TINY, synth.Scene()
    frames = list(synth.sequence(cam, scene, 24))
    ff_h = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=65536, flags=api.DSM_FLAG_UPLOAD_STREAM)
    ff_d = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=65536)
    ff_h.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    ff_d.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    orc = ob.PortOracle(cam)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for t, img, dep, pose, ref in frames:
        ti, td = torch.from_numpy(img.copy()).cuda(), torch.from_numpy(dep.copy()).cuda()
        torch.cuda.synchronize()
        ff_h.frame_upload(t & 1, img, dep)
        ff_d.frame_upload_device(t & 1, ti.data_ptr(), cam.width, td.data_ptr(), cam.width * 4)
        ff_h.fuse_frame_resident(t & 1, ref, pose)   # no synchronisation: the next upload overlaps this frame
        ff_d.fuse_frame_resident(t & 1, ref, pose)
        lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
    want = lo.astype(api.SURFEL_DTYPE)
    assert fields_equal(ff_h.map_download(), want) == []
    assert fields_equal(ff_d.map_download(), want) == []
    ff_h.close()
    ff_d.close()


def test_compaction_with_many_holes(mods):
    """Maps whose surfels are mostly stale (pruned this frame): the K < k branch with tail holes."""
    api, synth, ob = mods
    cam, scene = synth.TINY, synth.Scene()
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=65536)
    orc = ob.PortOracle(cam)
    rng = np.random.default_rng(11)
    seq = list(synth.sequence(cam, scene, 6))
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for t, img, dep, pose, ref in seq[:5]:
        lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
    for trial in range(8):
        m = lo.copy()
        stale = rng.random(len(m)) < rng.uniform(0.1, 0.9)
        m["last_update"][stale] = -100  # ref - last_update > 5
        m["update_times"][stale] = rng.integers(1, 5, int(stale.sum()))
        t, img, dep, pose, ref = seq[5]
        g, kg = ff.fuse_map(ref, img, dep, pose, m.astype(api.SURFEL_DTYPE))
        o, ko = orc.fuse_map(ref, img, dep, pose, m)
        assert kg == ko and len(g) == len(o), f"trial {trial}"
        assert not fields_equal(g, o.astype(api.SURFEL_DTYPE)), f"trial {trial}"
        assert (g["update_times"] != 0).all()


def test_out_of_domain_depth_is_reported(mods):
    """Depths of a few centimetres push every SLIC cost past the reference's 1e6 sentinel; the
    reference then reads superpixel_seeds[-1].  The HIP path reports DSM_E_INVALID instead."""
    api, synth, ob = mods
    cam = synth.TINY
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=65536)
    img = np.full((cam.height, cam.width), 90, np.uint8)
    dep = np.full((cam.height, cam.width), 5.0, np.float32)
    dep[::3, ::5] = 0.011
    with pytest.raises(api.DsmError) as ei:
        ff.fuse_map(0, img, dep, np.eye(4, dtype=np.float32), np.zeros(0, api.SURFEL_DTYPE))
    assert ei.value.code == -1


def test_full_size_properties(mods):
    """Size-independent properties at BASELINE's full sizes (no oracle): determinism, graph == eager,
    labels in range and local, no deleted slot survives compaction, count identity."""
    api, synth, ob = mods
    for cam in (synth.KITTI_1226, synth.FULLHD):
        scene = synth.Scene(seed=21)
        n = 6
        frames = list(synth.sequence(cam, scene, n))
        results = []
        for flags in (0, 0, 1):
            ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=1 << 20, flags=flags)
            for t, img, dep, pose, ref in frames:
                ff.frame_upload(t, img, dep)
            ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
            sizes = []
            for t, img, dep, pose, ref in frames:
                before = ff.map_size()
                ff.fuse_frame_resident(t, ref, pose)
                after, k = ff.map_size(), ff.last_new_count()
                sizes.append((before, k, after))
                assert after <= before + k
            m = ff.map_download()
            lab = ff.labels()
            results.append((m.tobytes(), lab.tobytes(), sizes))
            assert (m["update_times"] != 0).all()
            gw, gh = cam.width // 8, cam.height // 8
            assert lab.min() >= 0 and lab.max() < gw * gh
            ys, xs = np.mgrid[0:cam.height, 0:cam.width]
            assert (np.abs((lab % gw) * 8 + 4 - xs) < 8).all() and (np.abs((lab // gw) * 8 + 4 - ys) < 8).all()
            ff.close()
        assert results[0] == results[1], "two identical runs differ"
        assert results[0] == results[2], "graph replay and eager launch differ"


def test_golden_fixture(mods):
    """Committed vectors generated from the reference's own translation unit (tests/golden/make_golden.py)."""
    api, synth, ob = mods
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
    for case in meta["cases"]:
        cam = getattr(synth, case["camera"])
        scene = synth.Scene(**case["scene"])
        ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 20)
        lg = np.zeros(0, api.SURFEL_DTYPE)
        for (t, img, dep, pose, ref), want in zip(synth.sequence(cam, scene, case["frames"]), case["per_frame"]):
            lg, k = ff.fuse_map(ref, img, dep, pose, lg)
            assert k == want["n_new"] and len(lg) == want["n_local"], f"{case['name']} frame {t}"
            assert hashlib.sha256(ff.labels().tobytes()).hexdigest() == want["labels_sha256"], f"{case['name']} frame {t}"
        ref_map = np.load(os.path.join(ROOT, "tests", "golden", case["final_map"]))
        assert not fields_equal(lg, ref_map.astype(api.SURFEL_DTYPE)), case["name"]


def test_cpp_facade_parity(mods, oracle_built):
    """The C++ facade with the reference's class/method names, driven like surfel_map.cpp:1066-1109."""
    import subprocess
    from test_cpu import _build_facade_test
    exe = _build_facade_test(oracle_built)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def _random_rigid(rng, scale=0.05):
    a = rng.normal(size=3) * scale
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = rng.normal(size=3) * 0.3
    return m.astype(np.float32)


def _fused_map(mods, n_frames=6):
    api, synth, ob = mods
    cam, scene = synth.VGA_DRIVE, synth.Scene(seed=31)
    orc = ob.PortOracle(cam)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for t, img, dep, pose, ref in synth.sequence(cam, scene, n_frames):
        lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
    return cam, scene, orc, lo


def test_map_warp_matches_oracle(mods):
    """Loop-closure deformation of the resident (active) map, surfel_map.cpp:750-789."""
    api, synth, ob = mods
    cam, scene, orc, lo = _fused_map(mods)
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 20)
    rng = np.random.default_rng(5)
    for n in (len(lo), 1, 255, 256, 257, 1000):  # ragged tails of the 256-record blocks
        sub = lo[:n]
        warp = _random_rigid(rng)
        ff.map_upload(sub.astype(api.SURFEL_DTYPE))
        ff.map_warp(warp)
        got = ff.map_download()
        want = ob.port_warp(sub, warp).astype(api.SURFEL_DTYPE)
        assert not fields_equal(got, want), n
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    ff.map_warp(np.eye(4, dtype=np.float32))
    assert ff.map_size() == 0


def test_warp_grouped_device_matches_oracle(mods):
    """Per-keyframe deformation of detached surfels in caller-owned device memory, surfel_map.cpp:681-748."""
    import torch
    api, synth, ob = mods
    cam, scene, orc, lo = _fused_map(mods)
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1024)
    rng = np.random.default_rng(6)
    cuts = np.sort(rng.choice(np.arange(1, len(lo)), size=6, replace=False))
    offsets = np.concatenate([[0], cuts, [cuts[-1]], [len(lo)]]).astype(np.int32)  # includes an empty group
    mats = np.stack([_random_rigid(rng) for _ in range(len(offsets) - 1)])
    dev = torch.from_numpy(lo.view(np.uint8).copy()).cuda()
    ff.warp_grouped_device(dev.data_ptr(), offsets, mats)
    got = dev.cpu().numpy().view(api.SURFEL_DTYPE)
    want = lo.copy()
    for g in range(len(offsets) - 1):
        a, b = offsets[g], offsets[g + 1]
        want[a:b] = ob.port_warp(lo[a:b], mats[g])
    assert not fields_equal(got, want.astype(api.SURFEL_DTYPE))


def test_active_set_extract_append(mods):
    """move_add_surfels on the resident map (surfel_map.cpp:1476-1497, 1583-1590), then keep fusing."""
    api, synth, ob = mods
    cam, scene = synth.VGA_DRIVE, synth.Scene(seed=31)
    n = 12
    frames = list(synth.sequence(cam, scene, n))
    ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=1 << 20)
    orc = ob.PortOracle(cam)
    for t, img, dep, pose, ref in frames:
        ff.frame_upload(t, img, dep)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    parked = None
    for t, img, dep, pose, ref in frames:
        if t == 7:  # keyframe 0 leaves the active set
            lo, want = ob.port_extract_key(lo, 0)
            got = ff.map_extract(0)
            assert len(got) == len(want) > 0
            assert not fields_equal(got, want.astype(api.SURFEL_DTYPE))
            parked = got
        if t == 10:  # ... and comes back
            lo = np.concatenate([lo, parked.astype(ob.SURFEL_DTYPE)])
            ff.map_append(parked)
        ff.fuse_frame_resident(t, ref, pose)
        lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
        got_map = ff.map_download()
        assert not fields_equal(got_map, lo.astype(api.SURFEL_DTYPE)), t


def _seed_state_equal(ff, orc, tag):
    core, stable = ff.debug_get_seed_state()
    sd = orc.seeds()
    for k, f in enumerate(("x", "y", "mean_intensity", "mean_depth")):
        a, b = core[:, k], sd[f]
        same = (a.view("u4") == b.view("u4")) | (np.isnan(a) & np.isnan(b))
        assert same.all(), f"{tag}: seed field {f} differs at {np.nonzero(~same)[0][:5].tolist()}"
    assert np.array_equal(stable.astype(bool), sd["stable"].astype(bool)), f"{tag}: stable flags differ"


def test_state_level_early_return(mods):
    """State-level test of FF.cpp:516-517 on the GPU: after the first assignment, give all pixels of a few
    unstable superpixels to their neighbours, then run update_seeds on oracle and device.  The worker chunk
    of each victim must be abandoned from the victim on (k_update_seeds staging + k_commit_seeds)."""
    api, synth, ob = mods
    cam = synth.TINY
    img, dep, _ = synth.render(cam, synth.Scene(seed=8), 0)
    pose = np.eye(4, dtype=np.float32)
    gw = cam.width // 8
    rng = np.random.default_rng(0)
    for trial in range(5):
        ff = api.FusionFunctions.from_camera(cam, surfel_capacity=65536, flags=api.DSM_FLAG_NO_GRAPH)
        ff.frame_upload(0, img, dep)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        orc = ob.PortOracle(cam)
        orc.set_frame(img, dep)
        orc.stage("initialize_seeds")
        orc.stage("update_pixels")
        ff.debug_run_stages(0, 0, pose, "init_seeds", "assign_0")
        labels = ff.debug_get_labels(0)
        assert np.array_equal(labels, orc.labels())
        for victim in rng.choice(ff.n_seed, size=1 + trial, replace=False):
            victim = int(victim)
            neighbour = victim + 1 if (victim % gw) + 1 < gw else victim - 1
            labels[labels == victim] = neighbour  # the victim now owns nothing
        ff.debug_set_labels(0, labels)
        orc.set_labels(labels)
        ff.debug_run_stages(0, 0, pose, "update_seeds_0", "commit_seeds_0")
        orc.stage("update_seeds")
        _seed_state_equal(ff, orc, f"trial {trial} sweep 0")
        # and one more full sweep on top of the abandoned chunks
        ff.debug_run_stages(0, 0, pose, "assign_1", "commit_seeds_1")
        orc.stage("update_pixels")
        assert np.array_equal(ff.debug_get_labels(1), orc.labels()), trial
        orc.stage("update_seeds")
        _seed_state_equal(ff, orc, f"trial {trial} sweep 1")
        ff.close()


def test_state_level_stable_skip(mods):
    """State-level test of the sequential `stable` skip rule (FF.cpp:400,445,450): random stable flags on
    half of the superpixels, so that many pixels sit between two stable seeds and the worklist fixed point of
    k_assign / k_resolve has real work; labels and seeds after the sweep must equal the row-major scan's."""
    api, synth, ob = mods
    cam = synth.TINY
    pose = np.eye(4, dtype=np.float32)
    rng = np.random.default_rng(1)
    for trial in range(6):
        img, dep, _ = synth.render(cam, synth.Scene(seed=20 + trial, intensity_noise=60.0), trial)
        ff = api.FusionFunctions.from_camera(cam, surfel_capacity=65536, flags=api.DSM_FLAG_NO_GRAPH)
        ff.frame_upload(0, img, dep)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        orc = ob.PortOracle(cam)
        orc.set_frame(img, dep)
        orc.stage("initialize_seeds")
        orc.stage("update_pixels")
        orc.stage("update_seeds")
        ff.debug_run_stages(0, 0, pose, "init_seeds", "commit_seeds_0")
        _seed_state_equal(ff, orc, f"trial {trial} before")
        sd = orc.seeds()
        flags = rng.random(len(sd)) < (0.3 + 0.1 * trial)
        sd["stable"] = flags
        orc.set_seeds(sd)
        core, _ = ff.debug_get_seed_state()
        ff.debug_set_seed_state(core, flags.astype(np.int32))
        for sweep in (1, 2):
            ff.debug_run_stages(0, 0, pose, f"assign_{sweep}", f"commit_seeds_{sweep}")
            orc.stage("update_pixels")
            got, want = ff.debug_get_labels(sweep & 1), orc.labels()
            assert np.array_equal(got, want), f"trial {trial} sweep {sweep}: {int((got != want).sum())} labels differ"
            orc.stage("update_seeds")
            _seed_state_equal(ff, orc, f"trial {trial} sweep {sweep}")
        ff.close()


def test_inactive_store_matches_host_model(mods):
    """dsm_store_*: the device-side attached_surfels + inactive_pointcloud of surfel_map.cpp:1456-1595 / 681-748
    against the oracle's extract / warp on host arrays: deactivate in order, grouped warp with untouched and
    empty groups and the stale last point of every warped group, activate, erase with the tail moving down."""
    api, synth, ob = mods
    cam, scene, orc, local = _fused_map(mods, n_frames=12)
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 20)
    ff.map_upload(local.astype(api.SURFEL_DTYPE))
    rng = np.random.default_rng(3)
    store = np.zeros(0, ob.SURFEL_DTYPE)
    cloud = np.zeros((0, 4), np.float32)
    segs = []
    keys = [0, 5, 1, 2]  # keyframe 5 does not exist: an empty segment in the middle
    for key in keys:
        b, n = ff.store_deactivate(key)
        local, out = ob.port_extract_key(local, key)
        assert (b, n) == (len(store), len(out)), (key, b, n, len(store), len(out))
        segs.append((b, n))
        store = np.concatenate([store, out])
        cloud = np.concatenate([cloud, np.stack([out["px"], out["py"], out["pz"], out["color"]], axis=1).astype(np.float32)])
    assert sum(n for _, n in segs) > 1000 and segs[1][1] == 0
    assert fields_equal(ff.map_download(), local.astype(api.SURFEL_DTYPE)) == []

    def check(tag):
        s, c = ff.store_download()
        assert ff.store_size() == len(store), tag
        assert fields_equal(s, store.astype(api.SURFEL_DTYPE)) == [], tag
        assert np.array_equal(c.view("u4"), cloud.view("u4")), tag

    check("after deactivation")
    # loop closure: groups 0 and 3 move, 1 is empty, 2 stays
    offsets = np.array([b for b, _ in segs] + [len(store)], np.int32)
    mats = np.stack([_random_rigid(rng) for _ in keys])
    changed = np.array([1, 1, 0, 1], np.uint8)
    ff.store_warp(offsets, mats, changed)
    for g in range(len(keys)):
        if not changed[g]:
            continue
        b, e = offsets[g], offsets[g + 1]
        store[b:e] = ob.port_warp(store[b:e], mats[g])
        if e - b > 1:  # SM.cpp:742: [&front, &back) -- the last point of the patch keeps its old position
            cloud[b:e - 1] = np.stack([store["px"][b:e - 1], store["py"][b:e - 1], store["pz"][b:e - 1], store["color"][b:e - 1]], axis=1)
    check("after warp")
    # re-activate group 2 (keyframe 1), then erase it: the tail (group 3) moves down
    b2, n2 = segs[2]
    ff.store_activate(b2, n2)
    local = np.concatenate([local, store[b2:b2 + n2]])
    ff.store_erase(b2, n2)
    store = np.concatenate([store[:b2], store[b2 + n2:]])
    cloud = np.concatenate([cloud[:b2], cloud[b2 + n2:]])
    check("after erase")
    assert fields_equal(ff.map_download(), local.astype(api.SURFEL_DTYPE)) == []
    with pytest.raises(api.DsmError):
        ff.store_erase(len(store) - 1, 5)
    with pytest.raises(api.DsmError):
        ff.store_warp(offsets, mats, changed)  # offsets no longer tile the store
    ff.close()


def test_node_matches_reference_node(mods):
    """The whole node (message callbacks -> pose graph -> active / inactive sets -> per-frame engine -> loop-closure
    warp -> PCD / PLY export) on the GPU against the golden record of the reference's own surfel_map.cpp
    (tests/golden/make_node_golden.py): every keyframe pose, surfel, inactive point and exported byte."""
    import test_cpu
    from densesurfelmapping_amd import surfel_map
    for case, gold in test_cpu._node_cases():
        test_cpu._check_node_run(case, gold, lambda cam, d: surfel_map.SurfelMap(cam, drift_free_poses=d))


def test_reference_ros_node_on_the_product(mods, ros_node_on_product, tmp_path):
    """The reference's ros_node.cpp, compiled unchanged against include/ros_compat (exact ROS callback signatures, the
    SurfelMap(ros::NodeHandle&) constructor reading the nine parameters), pumping a recorded message stream through its
    own subscriber wiring: the PCD and PLY its main() saves at exit are the reference node's, byte for byte."""
    import subprocess
    import node_state
    import test_cpu
    api, synth, ob = mods
    case, gold = test_cpu._node_cases()[0]
    log = str(tmp_path / "events.bin")
    test_cpu._write_node_events(log, synth.NODE_CAM, case, synth)
    env = dict(os.environ, DSM_ROS_SHIM_LOG=log, DSM_ROS_SHIM_SAVE_NAME=str(tmp_path / "map"))
    r = subprocess.run([ros_node_on_product], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    for kind, path in (("pcd", str(tmp_path / "map.PCD")), ("ply", str(tmp_path / "map_mesh.PLY"))):
        got = node_state.file_digest(path)
        assert got["head"] == gold["files"][kind]["head"] and got["sha256"] == gold["files"][kind]["sha256"], kind


def test_reference_node_on_the_hip_engine(mods, ref_map_on_product):
    """INTEGRATION.md §2 end to end: the reference's own surfel_map.cpp (compiled in place, unchanged) with
    `FusionFunctions` = the product's facade, i.e. its fuse_map calls dsm_fuse_initialize_map on the GPU every frame and
    keeps its own refill / compaction loop.  Every keyframe pose, surfel, inactive point and exported byte equals the
    golden record of the all-CPU reference node."""
    import test_cpu
    api, synth, ob = mods
    for case, gold in test_cpu._node_cases():
        if case.get("camera") == "NODE_CAM_RGBD":
            continue  # the reference's initialize() has no way to select its commented-out RGB-D constant set
        test_cpu._check_node_run(case, gold, lambda cam, d: ob.RefSurfelMap(cam, drift_free_poses=d, lib_path=ref_map_on_product))


def test_cpp_surfel_map_wrapper_replay(mods, tmp_path):
    """include/dsm_surfel_map.hpp (the reference's class / callback names over plain message structs) replaying a
    recorded message stream: the PCD and PLY it saves are the reference node's, byte for byte."""
    import subprocess
    import node_state
    import test_cpu
    api, synth, ob = mods
    exe = test_cpu._build_node_replay_test()
    case, gold = test_cpu._node_cases()[0]
    ev, pcd, ply = str(tmp_path / "events.bin"), str(tmp_path / "map.PCD"), str(tmp_path / "map_mesh.PLY")
    test_cpu._write_node_events(ev, synth.NODE_CAM, case, synth)
    r = subprocess.run([exe, ev, pcd, ply], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for kind, path in (("pcd", pcd), ("ply", ply)):
        got = node_state.file_digest(path)
        assert got["head"] == gold["files"][kind]["head"] and got["sha256"] == gold["files"][kind]["sha256"], kind


def test_message_log_replay_driver(mods, tmp_path):
    """python -m densesurfelmapping_amd.msglog: a recorded message log replayed through the Python node, exports equal
    to the reference node's."""
    import node_state
    import test_cpu
    from densesurfelmapping_amd import msglog
    api, synth, ob = mods
    case, gold = test_cpu._node_cases()[1]
    log, pcd, ply = str(tmp_path / "log.bin"), str(tmp_path / "m.PCD"), str(tmp_path / "m.PLY")
    test_cpu._write_node_events(log, synth.NODE_CAM, case, synth)
    out = msglog.replay(log, save_cloud=pcd, save_mesh=ply)
    assert [out["frames_fused"], out["keyframes"], out["active_surfels"], out["inactive_surfels"]] == gold["briefs"][-1]
    for kind, path in (("pcd", pcd), ("ply", ply)):
        assert node_state.file_digest(path)["sha256"] == gold["files"][kind]["sha256"], kind


def _bench_line(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # the contract is ONE line on stdout, and stdout is a pipe here: what a native library left in libc's buffer (RCCL's
    # banner) would come out after the JSON at exit
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    return json.loads(lines[0])


def _kitti_layout(tmp_path, cam, scene, n, synth):
    """a synthetic drive written in kitti_publisher's directory layout (tests/test_cpu.py::test_kitti_layout_reader)"""
    import struct
    import zlib
    from densesurfelmapping_amd import kitti
    seq = tmp_path / "sequences" / "00"
    (seq / "image_0").mkdir(parents=True)
    (seq / "depth_0").mkdir()

    def png(path, img):
        h, w = img.shape
        rows = b"".join(b"\x00" + img[y].tobytes() for y in range(h))
        def chunk(kind, body):
            return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
        open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                               chunk(b"IDAT", zlib.compress(rows)) + chunk(b"IEND", b""))
    with open(tmp_path / "poses.txt", "w") as f:
        for t in range(n):
            img, dep, pose = synth.render(cam, scene, t)
            png(str(seq / "image_0" / ("%06d.png" % t)), img)
            with np.errstate(divide="ignore"):
                np.save(str(seq / "depth_0" / ("%06d.npy" % t)), (kitti.BF_SEQ_00_02 / dep.astype(np.float64)).astype(np.float32))
            f.write(" ".join("%.17g" % v for v in pose.astype(np.float64)[:3].ravel()) + "\n")
    open(seq / "calib.txt", "w").write(f"P0: {cam.fx} 0 {cam.cx} 0 0 {cam.fy} {cam.cy} 0 0 0 1 0\n")
    return str(seq), str(tmp_path / "poses.txt")


@pytest.mark.parametrize("source", ["synthetic", "kitti"])
def test_sharded_replay_two_ranks_on_one_gpu(mods, tmp_path, source):
    """BASELINE configs[2] end to end through the product's own driver, `python -m densesurfelmapping_amd.replay --gpus 2`
    (two ranks sharing this box's one GPU, clouds merged over gloo): a sequence -- synthetic, or read from
    kitti_publisher's on-disk layout -- is cut in two, rank r replays frames [a_r, b_r) on the HIP engine with keyframe
    indices restarting at 0, frames streamed from the host through two slots.  Every shard's map equals the oracle's
    for the same frames, byte for byte, and the merged cloud is the shards in rank order."""
    import subprocess
    import sys
    api, synth, ob = mods
    from densesurfelmapping_amd import replay
    n, out = 27, tmp_path / "out"
    if source == "synthetic":
        src = replay.SyntheticSource(n, camera="TINY", seed=31)
        what = ["--synthetic", str(n), "--camera", "TINY", "--seed", "31"]
    else:
        seq, poses = _kitti_layout(tmp_path, synth.NODE_CAM, synth.Scene(seed=9), n, synth)
        src = replay.KittiSource(seq, poses)
        assert src.n_frames == n and (src.cam.width, src.cam.fx) == (synth.NODE_CAM.width, synth.NODE_CAM.fx)
        what = ["--kitti", seq, "--poses", poses]
    r = subprocess.run([sys.executable, "-m", "densesurfelmapping_amd.replay"] + what +
                       ["--gpus", "2", "--one-device", "--backend", "gloo", "--save-shards", str(out), "--out", str(out / "merged.npy")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    head = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    shards = replay.shard_subsequences(n, 2)
    assert head["shards"] == [list(s) for s in shards] and head["world"] == 2
    parts = []
    for rank, (a, b) in enumerate(shards):
        orc, lo = ob.PortOracle(src.cam), np.zeros(0, ob.SURFEL_DTYPE)
        for k, (img, dep, pose) in enumerate(src.frames(a, b)):
            lo, _ = orc.fuse_map(k // 5, img, dep, pose, lo)
        got = np.load(out / f"shard_{rank}.npy")
        assert len(lo) > 0 and not fields_equal(got, lo.astype(api.SURFEL_DTYPE)), f"shard {rank}: frames [{a}, {b})"
        parts.append(got)
    merged = np.load(out / "merged.npy")
    assert merged.tobytes() == b"".join(p.tobytes() for p in parts) and head["counts"] == [len(p) for p in parts]
    assert head["merged_sha256"] == hashlib.sha256(merged.tobytes()).hexdigest()


@pytest.mark.parametrize("depth", [1, 4])
def test_async_uploads_between_frame_by_frame_and_chunked_enqueues(mods, depth):
    """The two orderings of dsm_frame(s)_upload_async on one handle, mixed: frames enqueued one at a time
    (dsm_fuse_frame_resident: the library does not list what they read, so the next upload waits for everything enqueued so
    far) and in chunks (dsm_replay_enqueue: an upload waits for the newest call that reads its slots), slots reused at once,
    no host wait anywhere -- a frame must never see the upload that follows it, nor miss the one before it.  Against the
    oracle, byte for byte."""
    api, synth, ob = mods
    cam, scene = synth.TINY, synth.Scene(seed=77)
    n = 40
    frames = list(synth.sequence(cam, scene, n))
    ff = api.FusionFunctions.from_camera(cam, frame_slots=4, surfel_capacity=1 << 17, pipeline_depth=depth)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    pin = api.PinnedFrames(ff, n)
    for t, img, dep, pose, ref in frames:
        pin.set(t, img, dep)
    t = 0
    while t < n:
        if (t // 8) % 2 == 0:  # one frame at a time through two slots in turn
            for _ in range(min(8, n - t)):
                ff.frame_upload_async(t & 1, pin.image(t), pin.depth(t))
                ff.fuse_frame_resident(t & 1, frames[t][4], frames[t][3])
                t += 1
        else:  # chunks of four through all four slots, the next chunk sent before this one is enqueued would need eight: here
            # every chunk overwrites the slots of the one before it -- the upload must wait for that one's frames
            for _ in range(2):
                m = min(4, n - t)
                if m <= 0:
                    break
                ff.frames_upload_async(0, pin, t, m)
                ff.replay_enqueue(*ff.pack_replay(list(range(m)), [f[4] for f in frames[t:t + m]], [f[3] for f in frames[t:t + m]]))
                t += m
    got = ff.map_download()
    ff.frame_uploads_wait()
    orc, lo = ob.PortOracle(cam), np.zeros(0, ob.SURFEL_DTYPE)
    for _, img, dep, pose, ref in frames:
        lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
    assert len(got) == len(lo) and not fields_equal(got, lo.astype(api.SURFEL_DTYPE))
    assert np.array_equal(ff.labels(), orc.labels())
    pin.close()
    ff.close()


@pytest.mark.parametrize("depth,chunk", [(24, 16), (1, 5), (8, 24)])
def test_replay_engine_streams_in_chunks(mods, depth, chunk):
    """replay.HipEngine.replay -- what a rank of the sharded replay runs on its shard: frames streamed from page-locked
    memory chunk by chunk (upload of chunk k+1 beside the kernels of chunk k, three groups of frame slots in turn), through frame groups
    -- over many chunks with a ragged last one, from a source whose frames are copied into the engine's page-locked blocks
    by the prefetch thread and from one that keeps them page-locked itself; a second replay on the same engine continues
    the sequence.  The map equals the oracle's for the same frames, byte for byte."""
    api, synth, ob = mods
    from densesurfelmapping_amd import replay
    n, start = 131, 7
    for prerender in (False, True):
        src = replay.SyntheticSource(start + n, camera="TINY", seed=31, prerender=prerender)
        eng = replay.HipEngine(src.cam, capacity=1 << 18, pipeline_depth=depth, chunk=chunk)
        cut = start + 3 * chunk + 1
        assert eng.replay(src, start, cut) == cut - start
        orc, lo = ob.PortOracle(src.cam), np.zeros(0, ob.SURFEL_DTYPE)
        for k, (img, dep, pose) in enumerate(src.frames(start, cut)):
            lo, _ = orc.fuse_map(k // 5, img, dep, pose, lo)
        assert eng.stats["zero_copy"] == prerender and eng.stats["frames"] == cut - start
        assert not fields_equal(eng.cloud(), lo.astype(api.SURFEL_DTYPE)), (prerender, "first replay")
        # ... and on: the same engine, keyframe indices restarting at 0 as replay() defines them
        eng.replay(src, cut, start + n)
        for k, (img, dep, pose) in enumerate(src.frames(cut, start + n)):
            lo, _ = orc.fuse_map(k // 5, img, dep, pose, lo)
        got = eng.cloud()
        assert len(got) == len(lo) and not fields_equal(got, lo.astype(api.SURFEL_DTYPE)), (prerender, "second replay")
        eng.close()
        src.close()


@pytest.mark.parametrize("world,workload", [(2, "headline"), (3, "headline"), (2, "sharded"), (3, "sharded")])
def test_bench_ranks_on_one_gpu(world, workload):
    """bench.py's multi-rank paths (sharding, barriers, max-over-ranks timing, all-gather merge) with two ranks, and with
    three, sharing the one GPU of the test box; collectives on gloo (the driver runs the real thing on RCCL).  Launched
    the way a user would: `python bench.py --gpus N` starts its own ranks.  `headline`: the weak-scaled batched replay;
    `sharded`: BASELINE configs[2] itself -- one sequence cut into one streamed subsequence per rank.  A multi-rank line is
    checked like a one-rank line, on EVERY rank: maps the TIMED run left behind against the CPU oracle's replay of the same frames
    (rank 0 one subsequence per batch, the other ranks one each; sharded: every rank its shard), the verdicts gathered."""
    import subprocess
    import sys
    env = dict(os.environ, DSM_BENCH_BACKEND="gloo", DSM_BENCH_ONE_DEVICE="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    if workload == "headline":
        extra = ["--steps", "20" if world == 2 else "6", "--warmup", "5" if world == 2 else "2", "--streams", "2", "--frames-per-step", "4"]
    else:
        extra = ["--workload", "sharded", "--steps", "3", "--warmup", "1", "--frames-per-step", "24" if world == 2 else "13", "--no-roofline"]
    # (at most three ranks: with the test process and torch.distributed.run's agent that stays within the six processes
    # a shared machine lets hold one GPU)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--full"] + extra,
                       env=env, capture_output=True, text=True, timeout=900)
    out = _bench_line(r)
    assert out["n_gpus"] == world and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["final_surfels_all_ranks"] > 0
    assert out["config"]["workload"].startswith("BASELINE configs[1]" if workload == "headline" else "BASELINE configs[2]")
    assert "cpu_baseline" not in out  # rank 0 at N=1 only
    mg = out["multi_gpu"]
    assert mg["world_size_seen_by_backend"] == world and len(mg["per_rank_frames_per_s"]) == world and mg["backend"] == "gloo"
    assert mg["min_rank_frames_per_s"] <= mg["max_rank_frames_per_s"] and mg["final_cloud_all_gather_ms"] > 0
    # value is the whole job over the slowest rank's time: never more than the sum of the ranks' own rates
    assert out["value"] <= sum(mg["per_rank_frames_per_s"]) * 1.001
    assert out["verified"] is True and out["verified_timed_region"] is True, out.get("verification")
    ranks = out["verification"]["ranks"]  # every rank checked a map of its own against the oracle, not only rank 0
    assert [r_["rank"] for r_ in ranks] == list(range(world)) and all(r_["equal"] is True and r_["surfels"] == r_["oracle_surfels"] > 0 for r_ in ranks), ranks
    if workload == "sharded":
        assert len(mg["per_rank_surfels"]) == world and min(mg["per_rank_surfels"]) > 0 and len(out["config"]["shards"]) == world


def test_hardware_reciprocal_is_within_one_ulp(tmp_path):
    """k_assign's filtered pick takes 1 / depth from v_rcp_f32 and prices its error into the bound (dsm_math.h: within one ulp of
    the correctly rounded quotient, a denormal quotient possibly flushed to 0 -- an absolute error below 2^-126).  Walked over
    EVERY float depth the reference gives an inverse depth to ((double)d > 0.01, FF.cpp:404), +inf included, on this GPU."""
    import shutil
    import subprocess
    exe = os.path.join(ROOT, "tests", "_build", "rcp_ulp")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc):
        exe = str(tmp_path / "rcp_ulp")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "rcp_ulp.hip"), "-o", exe],
                       check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    print("v_rcp_f32 against the correctly rounded quotient:", rec)
    assert rec["floats"] > 1_000_000_000 and rec["max_ulp_normal"] <= 1, rec
    assert rec["denormal_err_max_in_2^-149"] <= 1 << 23, rec  # (below 2^-126 whatever the hardware does with a denormal quotient)


_RCCL_WORKER = r"""
import json, sys, time, torch
sys.path.insert(0, sys.argv[1])
from densesurfelmapping_amd import replay
dist = replay.init_collective("nccl", 1, 0, 0)
assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
out = {}
for name, n in (("small", 1000), ("empty", 0), ("2GB", 48_000_000)):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(n + 1)
    cloud = torch.randint(0, 256, (n * 44,), dtype=torch.uint8, device="cuda:0", generator=g)
    replay.merge_clouds(cloud)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    merged, counts = replay.merge_clouds(cloud)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert counts == [n] and merged.numel() == n * 44 and merged.is_cuda and torch.equal(merged, cloud)
    out[name] = {"surfels": n, "bytes": n * 44, "ms": round(dt * 1e3, 3)}
dist.destroy_process_group()
print(json.dumps(out))
"""


def test_merge_clouds_through_rccl_on_one_gpu(tmp_path):
    """The final merge of BASELINE configs[2] through RCCL itself (backend "nccl" of torch.distributed on ROCm), in a process
    group of ONE on the test box's one GPU: the all-gather of the counts and of the padded cloud on DEVICE tensors -- a small
    cloud, an empty one (every rank empty: nothing is gathered), and a 2 GB one.  Then the two drivers the way a user starts
    them at --gpus 1: the replay CLI with --merge-at-world1, and bench.py, whose line names the backend that merged its clouds."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DSM_BENCH_ONE_DEVICE", "DSM_BENCH_BACKEND")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    script = tmp_path / "rccl_worker.py"
    script.write_text(_RCCL_WORKER)
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["2GB"]["bytes"] > 2_000_000_000 and rec["empty"]["surfels"] == 0
    print("merge_clouds over RCCL, world 1:", rec)
    r = subprocess.run([sys.executable, "-m", "densesurfelmapping_amd.replay", "--synthetic", "60", "--camera", "TINY", "--gpus", "1", "--merge-at-world1"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    head = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert head["backend"] == "nccl" and head["merged_surfels"] == head["surfels"] > 0 and head["counts"] == [head["surfels"]]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--streams", "8", "--batches", "1",
                        "--frames-per-step", "8", "--full", "--no-roofline", "--no-dropin", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900)
    out = _bench_line(r)
    mg = out["multi_gpu"]
    assert mg["backend"] == "nccl" and mg["world_size_seen_by_backend"] == 1 and mg["final_cloud_all_gather_ms"] > 0, mg
    assert mg["final_cloud_bytes_all_ranks"] == 44 * out["config"]["final_surfels_all_ranks"] > 0
    assert out["verified"] is True and out["verified_timed_region"] is True


def test_cpp_merge_clouds_through_rccl(tmp_path):
    """include/dsm_merge.h, the merge of BASELINE configs[2] for a C++ host: tests/cpp/merge_rccl_test.cpp creates an RCCL
    communicator of one (ncclCommInitRank) on the test box's GPU and merges a small cloud, an empty one and a 2 GB one through
    dsm_merge_clouds_rccl -- all-gather of the counts, all-gather of the padded cloud -- and checks capacity and argument errors."""
    import shutil
    import subprocess
    from densesurfelmapping_amd import build
    exe = os.path.join(ROOT, "tests", "_build", "merge_rccl_test")
    if os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        exe = build.build_merge_test(str(tmp_path / "merge_rccl_test"))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print("dsm_merge_clouds_rccl, world 1:", rec)
    assert rec["surfels_2GB"] * 44 > 2_000_000_000 and 0 < rec["ms_2GB"] < 1000


def test_bench_sharded_workload_one_gpu():
    """`bench.py --workload sharded` at --gpus 1: BASELINE configs[2]'s own path on one rank -- one subsequence streamed from
    page-locked host memory through one handle -- with its final map checked against the CPU oracle's replay of the same 192
    frames, the merge through RCCL (a group of one), a roofline and a CPU baseline in the line."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DSM_BENCH_ONE_DEVICE", "DSM_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "sharded", "--steps", "3", "--warmup", "1", "--full"],
                       env=env, capture_output=True, text=True, timeout=900)
    out = _bench_line(r)
    assert out["config"]["workload"].startswith("BASELINE configs[2]") and out["config"]["timed_frames_per_rank"] == 144
    assert out["verified_timed_region"] is True and out["verification"]["equal"] is True and out["verification"]["surfels"] > 10000
    assert out["multi_gpu"]["backend"] == "nccl" and out["roofline"]["frac"] > 0 and out["cpu_baseline"]["value"] > 0


def test_bench_dump_outputs_are_repeatable(tmp_path):
    """`bench.py --dump-outputs DIR` writes the final maps the timed steps left (a fixed sample of subsequences, float32
    (n, 11) in SURFEL_DTYPE field order and the codes of their non-finite fields, all finite, at most 64 MB), and two runs with the same arguments write the same arrays;
    --steps sets the number of timed steps and ms_per_step is the time of one."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DSM_BENCH_ONE_DEVICE", "DSM_BENCH_BACKEND")}
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--streams", "8", "--batches", "2",
                            "--frames-per-step", "4", "--no-roofline", "--no-dropin", "--no-cpu-baseline", "--no-verify", "--no-rccl-world1",
                            "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=900)
        out = _bench_line(r)
        assert out["steps"] == 3 and out["config"]["timed_frame_indices"] == [4, 15]
        assert abs(out["ms_per_step"] * 3 - out["config"]["timed_seconds"] * 1e3) < 0.01 * out["ms_per_step"] + 1e-3
        files = sorted(os.listdir(d))
        maps = [f for f in files if not f.endswith("_nonfinite.npy")]
        assert maps and all(f.startswith("map_s") and f.endswith(".npy") for f in files), files
        assert files == sorted(maps + [f[:-4] + "_nonfinite.npy" for f in maps]), files
        arrays = {f: np.load(d / f) for f in files}
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
        for f in maps:
            a, code = arrays[f], arrays[f[:-4] + "_nonfinite.npy"]
            assert a.ndim == 2 and a.shape[1] == 11 and len(a) > 0 and code.shape == (len(a),)
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for f in dumps[0]:
        assert dumps[0][f].tobytes() == dumps[1][f].tobytes(), f


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """`bench.py` without --full measures the headline and nothing else: its line has the headline's fields and none of what
    --full adds (per-kernel and roofline figures, the legs, the CPU baseline, the oracle's verdict, the merge at --gpus 1),
    and its dumped maps are those of a --full run with the same arguments."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DSM_BENCH_ONE_DEVICE", "DSM_BENCH_BACKEND")}
    args = ["--steps", "2", "--warmup", "1", "--streams", "8", "--batches", "2", "--frames-per-step", "4"]
    lines = {}
    for mode in ("plain", "full"):
        extra = [] if mode == "plain" else ["--full", "--no-roofline", "--no-dropin", "--no-cpu-baseline"]
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + extra + ["--dump-outputs", str(tmp_path / mode)],
                           env=env, capture_output=True, text=True, timeout=900)
        lines[mode] = _bench_line(r)
    out = lines["plain"]
    assert out["metric"] == "depth frames fused/sec @ KITTI 1226x370" and out["unit"] == "frames/s" and out["dtype"] == "f32"
    assert out["higher_is_better"] is True and out["value"] > 0 and out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    extras = {"roofline", "kernel_us", "cpu_baseline", "verification", "verified", "single_sequence", "dropin_pcie_inclusive",
              "fullhd_2M", "kitti_like", "tum_like", "streamed_input", "bounded_map"}
    assert not extras & out.keys(), extras & out.keys()
    assert out["multi_gpu"]["backend"] is None and "--full" in out["multi_gpu"]["note"]
    full = lines["full"]
    assert full["verified"] is True and full["multi_gpu"]["backend"] == "nccl"
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files and files == sorted(os.listdir(tmp_path / "full"))
    for f in files:
        assert np.load(tmp_path / "plain" / f).tobytes() == np.load(tmp_path / "full" / f).tobytes(), f


def test_bench_refuses_more_gpus_than_visible():
    """`python bench.py --gpus N` on a box with fewer than N devices must fail loudly -- not run one GPU and print n_gpus 1."""
    import subprocess
    import sys
    import torch
    n = torch.cuda.device_count() + 1
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DSM_BENCH_ONE_DEVICE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and not any(l.startswith("{") for l in r.stdout.splitlines()), r.stdout[-500:]
    assert "visible GPUs" in r.stderr
    # ... and a launcher-provided world that disagrees with --gpus is refused as well
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1"],
                       env=env2, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_bench_two_gpus_rccl():
    """Two ranks through `python bench.py --gpus 2`, RCCL all-gather of the final clouds where two devices exist (one GPU
    each, the real thing).  On a box with one GPU the same command runs with both ranks on it and the collectives on gloo
    (RCCL takes one rank per device): the two-rank line, its merge and its check against the CPU oracle are asserted alike."""
    import subprocess
    import sys
    import torch
    two = torch.cuda.device_count() >= 2
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DSM_BENCH_ONE_DEVICE", "DSM_BENCH_BACKEND")}
    if not two:
        env.update(DSM_BENCH_BACKEND="gloo", DSM_BENCH_ONE_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--streams", "8",
                        "--batches", "1", "--frames-per-step", "8", "--full", "--no-roofline"], env=env, capture_output=True, text=True, timeout=900)
    out = _bench_line(r)
    mg = out["multi_gpu"]
    assert out["n_gpus"] == 2 and mg["backend"] == ("nccl" if two else "gloo") and mg["world_size_seen_by_backend"] == 2
    assert len(mg["per_rank_frames_per_s"]) == 2 and mg["final_cloud_bytes_all_ranks"] == 44 * out["config"]["final_surfels_all_ranks"] > 0
    assert out["verified"] is True and out["verified_timed_region"] is True, out.get("verification")
