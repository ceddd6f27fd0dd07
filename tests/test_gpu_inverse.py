"""Caller-supplied pose inverses (the *_inv entry points, include/dsm.h; FF.cpp:59) through every form of the frame pipeline.

The C++ facade (include/dsm_fusion_functions.hpp) calls dsm_fuse_initialize_map_inv / dsm_fuse_map_inv whenever the pose type
has an inverse(), so this is the path an integrator runs.  Every form stages the inverses with index arithmetic of its own --
stage_params_batch (one frame for the drop-in calls, through stage_params; resident replays in chunks of kParamRing / 2 over a
ring of kParamRing), enqueue_frames (the loop of dsm_replay_enqueue and dsm_replay_enqueue_host, the latter's frames advancing
with it), batch_stage (handle-major: handle j's frames start at j * n_frames) -- and the frame groups read them G at a time.  Each case here feeds the inverses of tests/inverse_cases.py (near-exact, wrong on purpose,
hostile) and compares the engine with PortOracle fed THE SAME inverses (dsmo_fuse_map_inv, pinned to the reference's own TU by
tests/test_cpu.py::test_port_takes_the_callers_inverse): label image, seed table, surfel array and new-surfel count, every
byte equal, NaN == NaN, after every frame where the form allows it, otherwise after every call.  Every case also checks that
the same frames without the inverses give another map, so it does exercise them.
"""
import concurrent.futures
import json
import os

import numpy as np
import pytest

import inverse_cases as IC
from conftest import ROOT, fields_equal
from test_gpu_adversarial import _check_record, _digest, _gpu_record

pytestmark = pytest.mark.gpu

CAMERAS = {"TINY": 40, "KITTI_1226": 20}  # frames per sequence


@pytest.fixture(scope="module")
def mods(oracle_built):
    import torch
    torch.cuda.init()
    from densesurfelmapping_amd import api, synth
    from oracle import bindings
    return api, synth, bindings


def _frames(synth, cam, seed, n, start=0):
    """[(image, depth, pose, ref)] of a synthetic drive (the scene repeats its images every 50 frames; the pose keeps moving)"""
    return [(img, dep, pose, ref) for t, img, dep, pose, ref in synth.sequence(cam, synth.Scene(seed=seed), n, start=start)]


def _oracle(ob, cam, frames, invs, every=1):
    """frames through one PortOracle, frame t with invs[t] (None: the closed form); the record of _gpu_record after every
    `every`-th frame and the last one ({frame: record}), and the final surfel array"""
    orc = ob.PortOracle(cam)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    recs = {}
    for t, (img, dep, pose, ref) in enumerate(frames):
        lo, k = orc.fuse_map(ref, img, dep, pose, lo, inv_pose=None if invs is None else invs[t])
        if t % every == every - 1 or t == len(frames) - 1:
            recs[t] = (k, len(lo), _digest(orc.labels()), _digest(orc.seeds()), _digest(lo))
    return recs, lo


def _oracles(ob, cam, jobs):
    # one oracle per job on threads (the C oracle keeps no global state, ctypes lets go of the GIL)
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        return list(ex.map(lambda j: _oracle(ob, cam, *j), jobs))


def _differs(a, b):
    return len(a) != len(b) or fields_equal(a, b) != []


def _mixed(invs, without):
    """invs with the frames in `without` given no inverse (the closed form)"""
    return [None if t in without else invs[t] for t in range(len(invs))]


def _inv_or_none(invs, lo, hi):
    sel = invs[lo:hi]
    if any(x is None for x in sel):
        assert all(x is None for x in sel)
        return None
    return np.stack(sel)


@pytest.fixture(scope="module")
def seq(mods):
    """(camera, family) -> (frames, inverses [n, 16], {mask: (records, final map)}, control final map); mask "all": every frame
    with its inverse, "mixed": the frames of _mixed_out without (the resident replays' middle call)"""
    api, synth, ob = mods
    cache = {}

    def get(camera, family):
        if (camera, family) not in cache:
            cam = getattr(synth, camera)
            n = CAMERAS[camera]
            frames = _frames(synth, cam, 31, n)
            invs = IC.inverses(family, [f[2] for f in frames], seed=17 + 10 * list(CAMERAS).index(camera) + IC.FAMILIES.index(family))
            (ra, la), (rm, lm), (_, lc) = _oracles(ob, cam, [(frames, list(invs)), (frames, _mixed(list(invs), _mixed_out(n))),
                                                             (frames, None)])
            assert _differs(la, lc) and _differs(lm, lc), f"{camera} {family}: the inverses change nothing"
            cache[camera, family] = (frames, invs, {"all": (ra, la), "mixed": (rm, lm)}, lc)
        return cache[camera, family]
    return get


def _mixed_out(n):
    """the frames the resident replays enqueue WITHOUT inverses: the middle of three calls"""
    a, b = _calls(n)[:2]
    return set(range(a, a + b))


def _calls(n):
    """three enqueue calls: 13 frames (a ragged group at G = 4 and 8), then roughly half the rest, then the rest"""
    a = 13
    b = (n - a) // 2
    return [a, b, n - a - b]


# ---------------------------------------------------------------------------------------------------------------------
# (1) the drop-in calls in the facade's order

def _caller_compaction(local, fresh):
    """SM.cpp:1077-1109 as written (what the reference node does with fuse_initialize_map's two outputs), on copies"""
    local = list(local.copy())
    holes = [i for i, s in enumerate(local) if s["update_times"] == 0]
    for f in fresh:
        if f["update_times"] == 0:
            continue
        if holes:
            local[holes.pop()] = f
        else:
            local.append(f)
    n = len(local)
    while holes:
        local[holes.pop()] = local[n - 1]
        n -= 1
    return np.array(local[:n], dtype=fresh.dtype) if n else np.zeros(0, fresh.dtype)


@pytest.mark.parametrize("family", IC.FAMILIES)
@pytest.mark.parametrize("camera", list(CAMERAS))
def test_dropin_facade_order(mods, seq, camera, family):
    """What the facade runs for a reference-style integrator: dsm_fuse_initialize_map_inv on every frame (SM.cpp:1066), the
    caller compacting (SM.cpp:1077-1109) -- local and new surfels, labels and seeds after every frame; then the same frames
    through dsm_fuse_map_inv on the caller's own array, which goes through the page-locked shadow and the delta download, with
    a caller edit in the middle.  Both equal the oracle fed the same inverses after every frame."""
    api, synth, ob = mods
    cam = getattr(synth, camera)
    frames, invs, want, control = seq(camera, family)
    n = len(frames)
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 18)
    orc = ob.PortOracle(cam)
    try:
        lo = np.zeros(0, api.SURFEL_DTYPE)
        for t, (img, dep, pose, ref) in enumerate(frames):
            g_local, g_new = ff.fuse_initialize_map(ref, img, dep, pose, lo, inv_pose=invs[t])
            o_local, o_new = orc.fuse_initialize_map(ref, img, dep, pose, lo.astype(ob.SURFEL_DTYPE), inv_pose=invs[t])
            assert fields_equal(g_local, o_local.astype(api.SURFEL_DTYPE)) == [], f"{camera} {family} frame {t}: local"
            assert fields_equal(g_new, o_new.astype(api.SURFEL_DTYPE)) == [], f"{camera} {family} frame {t}: new"
            assert _digest(ff.labels()) == _digest(orc.labels()) and _digest(ff.seeds()) == _digest(orc.seeds()), f"frame {t}"
            lo = _caller_compaction(g_local, g_new)
        # the caller's compaction is the oracle's fuse_map: the facade-order map is the "all" replay's
        assert _digest(lo) == want["all"][0][n - 1][4], f"{camera} {family}: facade-order map"
        assert _differs(lo, control.astype(api.SURFEL_DTYPE))
        st0 = ff.debug_dropin_stats()
    finally:
        ff.close()
    # dsm_fuse_map_inv on the caller's array: shadow + delta download
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 18)
    orc = ob.PortOracle(cam)
    try:
        buf = np.zeros(1 << 17, api.SURFEL_DTYPE)
        m, lo = 0, np.zeros(0, ob.SURFEL_DTYPE)
        for t, (img, dep, pose, ref) in enumerate(frames):
            if t == n // 2 and m:  # one record edited by the caller: the shadow must notice
                buf["pz"][m // 2] += 0.25
                lo["pz"][m // 2] += 0.25
            m, k = ff.fuse_map_inplace(ref, img, dep, pose, buf, m, inv_pose=invs[t])
            lo, ko = orc.fuse_map(ref, img, dep, pose, lo, inv_pose=invs[t])
            assert (k, m) == (ko, len(lo)), f"{camera} {family} frame {t}: counts {(k, m)} vs {(ko, len(lo))}"
            assert fields_equal(buf[:m], lo.astype(api.SURFEL_DTYPE)) == [], f"{camera} {family} frame {t}: surfels"
            assert _digest(ff.labels()) == _digest(orc.labels()) and _digest(ff.seeds()) == _digest(orc.seeds()), f"frame {t}"
        st = ff.debug_dropin_stats()
        assert st["calls"] == n and st["delta_calls"] > 0, st
        print(camera, family, "initialize_map calls", st0, "fuse_map calls", st)
    finally:
        ff.close()


# ---------------------------------------------------------------------------------------------------------------------
# (2) resident replays: one graph per frame (depth 1) and frame groups (depth 8: G = 4, depth 24: G = 8)

@pytest.mark.parametrize("family", IC.FAMILIES)
@pytest.mark.parametrize("depth", [1, 8, 24])
@pytest.mark.parametrize("camera", list(CAMERAS))
def test_replay_enqueue(mods, seq, camera, depth, family):
    """dsm_replay_enqueue_inv in three calls on one handle: with inverses (13 frames: a ragged group), WITHOUT (the closed form
    staged into the ring next to entries that came with one), with inverses again.  After each call the handle equals the
    oracle's record of that frame.  At 1226x370 the frame groups run the lane-per-seed kernels."""
    api, synth, ob = mods
    cam = getattr(synth, camera)
    frames, invs, want, control = seq(camera, family)
    n = len(frames)
    recs, final = want["mixed"]
    inv_list = _mixed(list(invs), _mixed_out(n))
    ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=1 << 20, pipeline_depth=depth)
    try:
        for t, (img, dep, _, _) in enumerate(frames):
            ff.frame_upload(t, img, dep)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        s, r, p = api.FusionFunctions.pack_replay(list(range(n)), [f[3] for f in frames], np.stack([f[2] for f in frames]))
        lo = 0
        for m in _calls(n):
            ff.replay_enqueue(s[lo:lo + m], r[lo:lo + m], p[lo:lo + m], inv_poses_cm=_inv_or_none(inv_list, lo, lo + m))
            ff.synchronize()
            lo += m
            _check_record(f"{camera} depth {depth} {family} frame {lo - 1}", _gpu_record(ff), recs[lo - 1])
        assert _differs(ff.map_download(), control.astype(api.SURFEL_DTYPE))
    finally:
        ff.close()


# ---------------------------------------------------------------------------------------------------------------------
# (3) host-frame replays

@pytest.mark.parametrize("family", IC.FAMILIES)
def test_replay_enqueue_host(mods, seq, family):
    """dsm_replay_enqueue_host with inverses at depth 8 (G = 4) and 1226x370, in two calls of 9 and 11 frames: ragged ends, the
    parameters written to the ring by the host-frame loop and copied up by the group / frame that runs them"""
    api, synth, ob = mods
    cam = synth.KITTI_1226
    frames, invs, want, control = seq("KITTI_1226", family)
    n = len(frames)
    recs, final = want["all"]
    ff = api.FusionFunctions.from_camera(cam, frame_slots=8, surfel_capacity=1 << 20, pipeline_depth=8)
    pin = api.PinnedFrames(ff, n)
    try:
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        for t, (img, dep, _, _) in enumerate(frames):
            pin.set(t, img, dep)
        _, refs, poses = api.FusionFunctions.pack_replay(list(range(n)), [f[3] for f in frames], np.stack([f[2] for f in frames]))
        first = 9
        ff.replay_enqueue_host(pin, 0, refs[:first], poses[:first], inv_poses_cm=invs[:first])
        ff.replay_enqueue_host(pin, first, refs[first:], poses[first:], inv_poses_cm=invs[first:])
        ff.replay_wait()
        ff.synchronize()
        _check_record(f"host frames {family} frame {n - 1}", _gpu_record(ff), recs[n - 1])
        assert fields_equal(ff.map_download(), final.astype(api.SURFEL_DTYPE)) == []
        assert _differs(ff.map_download(), control.astype(api.SURFEL_DTYPE))
    finally:
        pin.close()
        ff.close()


# ---------------------------------------------------------------------------------------------------------------------
# (4) a batch of eight handles

def test_batch_of_eight(mods):
    """dsm_batch_replay_enqueue_inv over eight handles at 1226x370 (the lane-per-seed kernels, k_seed_fit's short tier limit
    lowered so its full-length tier takes groups too), a frame per call: every handle its own scene, its own inverse family
    and seed.  Frames 5-7 go without inverses, the rest with them; handle-major staging means handle j's inverses start at
    j * n_frames in the call's array.  Every handle equals its oracle after every frame."""
    api, synth, ob = mods
    cam, n, B = synth.KITTI_1226, 12, 8
    without = {5, 6, 7}
    runs, invs = [], []
    for b in range(B):
        fr = _frames(synth, cam, 100 + 13 * b, n, start=3 * b)
        runs.append(fr)
        invs.append(_mixed(list(IC.inverses(IC.FAMILIES[b % 3], [f[2] for f in fr], seed=500 + b)), without))
    want = _oracles(ob, cam, [(runs[b], invs[b]) for b in range(B)] + [(runs[b], None) for b in range(B)])
    for b in range(B):
        assert _differs(want[b][1], want[B + b][1]), f"handle {b}: its inverses change nothing"
    handles, batch = [], None
    try:
        for fr in runs:
            ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=1 << 20, pipeline_depth=1)
            ff.debug_set_fit_small_cap(40)
            for t, (img, dep, _, _) in enumerate(fr):
                ff.frame_upload(t, img, dep)
            ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
            handles.append(ff)
        plans = [api.FusionFunctions.pack_replay(list(range(n)), [f[3] for f in fr], np.stack([f[2] for f in fr])) for fr in runs]
        batch = api.Batch(handles)
        tiers = []
        for t in range(n):
            s, r, p, m = api.Batch.pack([(pl[0][t:t + 1], pl[1][t:t + 1], pl[2][t:t + 1]) for pl in plans])
            inv = None if t in without else np.stack([invs[b][t] for b in range(B)])
            batch.replay_enqueue(s, r, p, m, inv_poses_cm=inv)
            batch.synchronize()
            tiers += [h.debug_tier_counts() for h in handles]
            for b, h in enumerate(handles):
                _check_record(f"batch handle {b} ({IC.FAMILIES[b % 3]}) frame {t}", _gpu_record(h), want[b][0][t])
        # the lane forms ran (only k_update_seeds queues seeds for more Huber passes) and k_seed_fit's full-length tier took groups
        assert any(any(tc["huber_rest_by_sweep"]) for tc in tiers), tiers
        assert max(tc["fit_long_groups"] for tc in tiers) > 0, tiers
    finally:
        if batch is not None:
            batch.close()
        for h in handles:
            h.close()


# ---------------------------------------------------------------------------------------------------------------------
# (5) the parameter ring: chunks of kParamRing / 2 = 2048 frames, wrap-around at kParamRing = 4096

PERIOD = 50  # synth.Scene: the images repeat every 50 frames (the poses do not): 50 resident slots hold any sequence


def _long_run(synth, cam, seed, n):
    frames = _frames(synth, cam, seed, n)
    return frames, [t % PERIOD for t in range(n)]


def test_ring_chunks_and_wrap_one_handle(mods):
    """One handle at TINY, depth 1, four calls: 500 frames without inverses (ring entries 0-499), 500 with near-exact ones
    (500-999), 3300 with wrong ones -- ONE call that crosses the 2048-frame chunk and the ring's wrap at 4096, its last frames
    restaging entries 0-203 that the closed form filled -- then 400 without, on entries 204-603, some of which came with an
    inverse.  Compared after every call."""
    api, synth, ob = mods
    cam = synth.TINY
    calls = [(500, None), (500, "near"), (3300, "wrong"), (400, None)]
    n = sum(c for c, _ in calls)
    frames, slots = _long_run(synth, cam, 61, n)
    inv_list, lo = [], 0
    for m, fam in calls:
        inv_list += [None] * m if fam is None else list(IC.inverses(fam, [f[2] for f in frames[lo:lo + m]], seed=lo + 1))
        lo += m
    ends = np.cumsum([c for c, _ in calls]) - 1
    (recs, final), (_, control) = _oracles(ob, cam, [(frames, inv_list, 100), (frames, None, n)])
    assert _differs(final, control)
    ff = api.FusionFunctions.from_camera(cam, frame_slots=PERIOD, surfel_capacity=1 << 18, pipeline_depth=1)
    try:
        for t in range(PERIOD):
            ff.frame_upload(t, frames[t][0], frames[t][1])
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        s, r, p = api.FusionFunctions.pack_replay(slots, [f[3] for f in frames], np.stack([f[2] for f in frames]))
        lo = 0
        for (m, fam), end in zip(calls, ends):
            ff.replay_enqueue(s[lo:lo + m], r[lo:lo + m], p[lo:lo + m], inv_poses_cm=_inv_or_none(inv_list, lo, lo + m))
            ff.synchronize()
            lo += m
            _check_record(f"ring, call ending at frame {end}", _gpu_record(ff), _rec_at(recs, end))
    finally:
        ff.close()


def _rec_at(recs, t):
    assert t in recs, (t, sorted(recs)[:4])
    return recs[t]


def test_ring_chunks_batch_of_two(mods):
    """A batch of two handles (each its own scene and inverse family) at TINY: one call of 2100 frames with inverses crosses
    the 2048-frame chunk (batch_stage stages frames [i0, i0 + m) of every handle from offset j * n_frames + i0), then 60
    frames without."""
    api, synth, ob = mods
    cam, n1, n2 = synth.TINY, 2100, 60
    n = n1 + n2
    runs, invs = [], []
    for b, fam in enumerate(("wrong", "near")):
        frames, slots = _long_run(synth, cam, 71 + b, n)
        runs.append((frames, slots))
        invs.append(list(IC.inverses(fam, [f[2] for f in frames[:n1]], seed=900 + b)) + [None] * n2)
    want = _oracles(ob, cam, [(runs[b][0], invs[b], 2100) for b in range(2)] + [(runs[b][0], None, n) for b in range(2)])
    for b in range(2):
        assert _differs(want[b][1], want[2 + b][1]), b
    handles, batch = [], None
    try:
        for frames, _ in runs:
            ff = api.FusionFunctions.from_camera(cam, frame_slots=PERIOD, surfel_capacity=1 << 18, pipeline_depth=1)
            for t in range(PERIOD):
                ff.frame_upload(t, frames[t][0], frames[t][1])
            ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
            handles.append(ff)
        plans = [api.FusionFunctions.pack_replay(sl, [f[3] for f in fr], np.stack([f[2] for f in fr])) for fr, sl in runs]
        batch = api.Batch(handles)
        for lo, hi in ((0, n1), (n1, n)):
            s, r, p, m = api.Batch.pack([(pl[0][lo:hi], pl[1][lo:hi], pl[2][lo:hi]) for pl in plans])
            inv = None if lo else np.concatenate([np.stack(invs[b][:n1]) for b in range(2)])  # handle-major, as the poses
            batch.replay_enqueue(s, r, p, m, inv_poses_cm=inv)
            batch.synchronize()
            for b, h in enumerate(handles):
                _check_record(f"batch of two, handle {b}, frame {hi - 1}", _gpu_record(h), _rec_at(want[b][0], hi - 1))
    finally:
        if batch is not None:
            batch.close()
        for h in handles:
            h.close()


# ---------------------------------------------------------------------------------------------------------------------
# (6) the inverses with DSM_FLAG_EIGEN33_PRODUCTS (the facade's combination under DSM_MATCH_CALLER_EIGEN)

def test_eigen33_flag_with_inverses(mods):
    """The Eigen >= 3.3 fixtures (tests/golden/make_golden_eigen33.py) recorded the TU's own Matrix4f inverse, which the C
    restatement cannot evaluate in that product order, so perturbed inverses under the flag are not pinned here.  What can be
    asserted: with the closed-form inverses handed in, the flagged handle reproduces the fixture through dsm_fuse_map_inv and
    through dsm_replay_enqueue_inv with frame groups; with wrong inverses it does not."""
    import eigen33_cases as E
    api, synth, ob = mods
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "eigen33_golden.json")))
    case = next(c for c in E.SEQUENCES if c["name"] == "tiny_ragged_40")
    g = next(x for x in gold["sequences"] if x["name"] == "tiny_ragged_40")
    cam = getattr(synth, case["camera"])
    frames = list(E.sequence(case, synth))
    exact = np.stack([IC.closed_form(f[3]) for f in frames])
    wrong = IC.inverses("wrong", [f[3] for f in frames], seed=33)
    flag = api.DSM_FLAG_EIGEN33_PRODUCTS
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 18, flags=flag)
    try:
        lg = np.zeros(0, api.SURFEL_DTYPE)
        for (t, img, dep, pose, ref), want in zip(frames, g["per_frame"]):
            lg, k = ff.fuse_map(ref, img, dep, pose, lg, inv_pose=exact[t])
            got = E.frame_record(k, lg, ff.labels(), ff.seeds())
            assert got == want, f"frame {t}: " + str({f: (got[f], want[f]) for f in got if got[f] != want[f]})
        assert E.final_map_differences(lg, g, os.path.join(ROOT, "tests", "golden")) == []
    finally:
        ff.close()
    for invs, same in ((exact, True), (wrong, False)):
        ff = api.FusionFunctions.from_camera(cam, frame_slots=len(frames), surfel_capacity=1 << 18, pipeline_depth=8, flags=flag)
        try:
            for t, img, dep, pose, ref in frames:
                ff.frame_upload(t, img, dep)
            ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
            s, r, p = api.FusionFunctions.pack_replay([f[0] for f in frames], [f[4] for f in frames], np.stack([f[3] for f in frames]))
            ff.replay_enqueue(s[:27], r[:27], p[:27], inv_poses_cm=invs[:27])
            ff.replay_enqueue(s[27:], r[27:], p[27:], inv_poses_cm=invs[27:])
            ff.synchronize()
            bad = E.final_map_differences(ff.map_download(), g, os.path.join(ROOT, "tests", "golden"))
            assert (bad == []) == same, ("closed-form" if same else "wrong", bad)
        finally:
            ff.close()
