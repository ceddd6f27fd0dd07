"""The label image of a sweep >= 1 is final where k_assign stores it (pixels whose old seed was unstable at sweep start) and
after k_resolve's walk over its list (the others): no pass over every pixel in between.  State level on one handle with
chosen stable flags, the lane forms of batches and frame groups in a scene where many seeds are stable, and a pixel
without a pick."""
import numpy as np
import pytest

from conftest import fields_equal
from test_gpu_parity import _compare_frame, _seed_state_equal, mods  # noqa: F401  (mods: the module fixture)

pytestmark = pytest.mark.gpu

POSE = np.eye(4, dtype=np.float32)


def _after_first_sweep(api, ob, cam, img, dep):
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=65536, flags=api.DSM_FLAG_NO_GRAPH)
    ff.frame_upload(0, img, dep)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    orc = ob.PortOracle(cam)
    orc.set_frame(img, dep)
    orc.stage("initialize_seeds")
    orc.stage("update_pixels")
    orc.stage("update_seeds")
    ff.debug_run_stages(0, 0, POSE, "init_seeds", "commit_seeds_0")
    return ff, orc


# ------------------------------------------------------------------------------------------------------ 1. state level
@pytest.mark.parametrize("stable", ["none", "half", "all"])
@pytest.mark.parametrize("camera", ["TINY", "TINY_RAGGED"])
def test_state_level_sweep_labels(mods, camera, stable):
    """Stable flags after sweep 0 set to none / a random half / all of the seeds; labels and seed state after each of sweeps
    1 and 2 equal the oracle's row-major scan.  The counts that keep the test from passing on nothing are taken on the
    oracle's side: labels before and after a sweep, and the flags the sweep started from."""
    api, synth, ob = mods
    cam = getattr(synth, camera)
    img, dep, _ = synth.render(cam, synth.Scene(seed=20, intensity_noise=60.0), 0)
    ff, orc = _after_first_sweep(api, ob, cam, img, dep)
    try:
        _seed_state_equal(ff, orc, f"{camera} before")
        sd = orc.seeds()
        rng = np.random.default_rng(5)
        flags = {"none": np.zeros(len(sd), bool), "half": rng.random(len(sd)) < 0.5, "all": np.ones(len(sd), bool)}[stable]
        sd["stable"] = flags
        orc.set_seeds(sd)
        core, _ = ff.debug_get_seed_state()
        ff.debug_set_seed_state(core, flags.astype(np.int32))
        changed, changed_stable = {}, {}
        for sweep in (1, 2):
            before, at_start = orc.labels().copy(), orc.seeds()["stable"].astype(bool)
            ff.debug_run_stages(0, 0, POSE, f"assign_{sweep}", f"commit_seeds_{sweep}")
            orc.stage("update_pixels")
            got, want = ff.debug_get_labels(0), orc.labels()
            assert np.array_equal(got, want), f"{camera} {stable} sweep {sweep}: {int((got != want).sum())} labels differ"
            orc.stage("update_seeds")
            _seed_state_equal(ff, orc, f"{camera} {stable} sweep {sweep}")
            moved = (want != before) & (before >= 0)
            changed[sweep] = int(moved.sum())
            changed_stable[sweep] = int((moved & at_start[np.maximum(before, 0)]).sum())
        print(camera, stable, "labels changed", changed, "of them with a stable old seed", changed_stable)
        if camera == "TINY_RAGGED":
            assert (want == -1).any() and (got == -1).sum() == (want == -1).sum()
        if stable == "none":
            assert changed[1] >= 1000 and changed_stable[1] == 0, (changed, changed_stable)
        elif stable == "half":
            assert changed_stable[1] >= 100 and changed_stable[2] >= 20, (changed, changed_stable)
        else:
            assert changed == {1: 0, 2: 0}, changed
    finally:
        ff.close()


# ------------------------------------------------------------------------------------------------------ 2. lane forms
QUIET = dict(intensity_noise=1.0, checker=4.0, depth_noise=0.0002, hole_fraction=0.002)  # test_quiet_scene_many_stable_seeds
N_QUIET = 12


@pytest.fixture(scope="module")
def quiet_oracle(mods):
    """Eight quiet scenes on TINY_RAGGED, twelve frames each: the frames, and per scene the oracle after the last frame, its
    map, and the largest number of stable seeds it saw at the end of a frame."""
    api, synth, ob = mods
    cam = synth.TINY_RAGGED
    runs, want = [], []
    for b in range(8):
        scene = synth.Scene(seed=3 + b, **QUIET)
        fr = [(img, dep, pose, ref) for _, img, dep, pose, ref in synth.sequence(cam, scene, N_QUIET)]
        orc = ob.PortOracle(cam)
        lo = np.zeros(0, ob.SURFEL_DTYPE)
        stable_seen = 0
        for img, dep, pose, ref in fr:
            lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
            stable_seen = max(stable_seen, int(orc.seeds()["stable"].sum()))
        runs.append(fr)
        want.append((orc, lo, stable_seen))
    return cam, runs, want


def _plan(api, fr):
    return api.FusionFunctions.pack_replay(list(range(len(fr))), [f[3] for f in fr], np.stack([f[2] for f in fr]))


def _upload(api, cam, fr, depth):
    ff = api.FusionFunctions.from_camera(cam, frame_slots=len(fr), surfel_capacity=1 << 18, pipeline_depth=depth)
    for t, (img, dep, _, _) in enumerate(fr):
        ff.frame_upload(t, img, dep)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    return ff


def _check_quiet(tag, api, ff, want):
    orc, lo, stable_seen = want
    assert stable_seen > ff.n_seed // 3, f"{tag}: the scene no longer produces many stable seeds ({stable_seen} of {ff.n_seed})"
    got = ff.map_download()
    assert fields_equal(got, lo.astype(api.SURFEL_DTYPE)) == [], tag
    _compare_frame(tag, ff, orc, got, lo.astype(api.SURFEL_DTYPE))  # (the last frame's label image and seed table too)


def test_quiet_scenes_batch_of_eight(mods, quiet_oracle):
    """Eight handles in lockstep (k_assign<false, true, 4>), most seeds stable from the second frame on: the list holds the
    borders between them, and k_resolve's walk over it decides their labels."""
    api, synth, ob = mods
    cam, runs, want = quiet_oracle
    handles, batch = [], None
    try:
        handles = [_upload(api, cam, fr, 1) for fr in runs]
        batch = api.Batch(handles)
        s, r, p, n = api.Batch.pack([_plan(api, fr) for fr in runs])
        batch.replay_enqueue(s, r, p, n)
        batch.synchronize()
        for b, ff in enumerate(handles):
            _check_quiet(f"batch handle {b}", api, ff, want[b])
    finally:
        if batch is not None:
            batch.close()
        for ff in handles:
            ff.close()


def test_quiet_scene_frame_groups_of_four(mods, quiet_oracle):
    """One handle with pipeline depth 16: the superpixel stages of four consecutive frames as one batched launch in the lane
    forms, three groups."""
    api, synth, ob = mods
    cam, runs, want = quiet_oracle
    ff = _upload(api, cam, runs[0], 16)
    try:
        slots, refs, poses = _plan(api, runs[0])
        ff.replay_enqueue(slots, refs, poses)
        ff.synchronize()
        _check_quiet("frame groups", api, ff, want[0])
    finally:
        ff.close()


# ------------------------------------------------------------------------------------------------------ 3. no pick
def test_pixel_without_a_pick_keeps_its_label(mods):
    """A depth of a centimetre pushes every candidate's cost past the reference's 1e6 sentinel (the frame of
    test_out_of_domain_depth_is_reported): in a sweep >= 1 such a pixel keeps its label and the stage reports it.  The
    pixels are chosen among those whose label the sweep changes when the depth is sound, and every other pixel's label is
    what it is in that sound sweep: a pick depends on no other pixel's depth, and with no seed stable the pick is the label."""
    api, synth, ob = mods
    cam = synth.TINY
    img, dep, _ = synth.render(cam, synth.Scene(seed=20, intensity_noise=60.0), 0)
    dep = np.where(dep > 1.0, dep, np.float32(5.0)).astype(np.float32)  # (every seed has a depth: no candidate is costed without it)
    sound, orc = _after_first_sweep(api, ob, cam, img, dep)
    ff, _ = _after_first_sweep(api, ob, cam, img, dep)
    try:
        before = sound.debug_get_labels(0)
        assert np.array_equal(before, ff.debug_get_labels(0))
        sound.debug_run_stages(0, 0, POSE, "assign_1", "resolve_1")
        after_sound = sound.debug_get_labels(0)
        moving = np.argwhere(after_sound != before)
        assert len(moving) >= 1000
        sel = moving[:: len(moving) // 40][:40]
        bad = np.zeros(dep.shape, bool)
        bad[sel[:, 0], sel[:, 1]] = True
        dep_bad = dep.copy()
        dep_bad[bad] = 0.011
        ff.frame_upload(0, img, dep_bad)  # (the same slot: the sweep reads the frame where init_seeds found it)
        with pytest.raises(api.DsmError) as ei:
            ff.debug_run_stages(0, 0, POSE, "assign_1", "resolve_1")
        assert ei.value.code == -1 and "1e6" in str(ei.value)
        got = ff.debug_get_labels(0)
        assert np.array_equal(got[bad], before[bad])
        assert np.array_equal(got, np.where(bad, before, after_sound))
    finally:
        sound.close()
        ff.close()
