"""k_seed_fit behind k_seed_stats takes its inliers from the row masks that kernel left (DeviceCtx::inl_mask) instead of deriving
them from labels and depths again; behind k_seed_points it still derives them.  Maps, label images and seed tables of every
launch form against the C restatement (PortOracle) after every frame, every byte equal (NaN == NaN), and the forms against
each other:

  1. a batch of eight handles at 166x103 (S = 240: the last wave of k_seed_stats is partial; ragged borders; windows leave
     the image on all four sides) and at 192x103 (the width is the pitch);
  2. the same batch with the short tier's limit at 0: every group goes through the queue tier, which finds its masks by seed;
  3. a scene of holes and depth edges in which seeds gain and lose their plane from frame to frame: the rows a seed left in
     an earlier frame are stale and must be ignored;
  4. one handle with frame groups of four (lane forms, masks) against the same handle frame by frame (wave forms, no masks);
  5. the Eigen >= 3.3 product order once through case 1 (launch_frame pairs the stages the same way with the flag)."""
import numpy as np
import pytest

import fit_mask_cases as F
from conftest import fields_equal
from test_gpu_parity import mods  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu


def _same_frame(tag, api, ff, want):
    k, lab, seeds, lo = want
    assert ff.last_new_count() == k, f"{tag}: new surfel count {ff.last_new_count()} vs {k}"
    got = ff.labels()
    assert np.array_equal(got, lab), f"{tag}: {int((got != lab).sum())} labels differ"
    bad = fields_equal(ff.seeds(), seeds)
    assert not bad, f"{tag}: seed table differs {bad}"
    loc = ff.map_download()
    assert len(loc) == len(lo), f"{tag}: surfel count {len(loc)} vs {len(lo)}"
    bad = fields_equal(loc, lo.astype(api.SURFEL_DTYPE))
    assert not bad, f"{tag}: surfels differ {bad}"


def _handle(api, cam, fr, depth=1, flags=0, fit_small_cap=None, constants=None):
    ff = api.FusionFunctions.from_camera(cam, frame_slots=len(fr), surfel_capacity=1 << 16, pipeline_depth=depth, flags=flags,
                                         constants=constants)
    if fit_small_cap is not None:
        ff.debug_set_fit_small_cap(fit_small_cap)
    for t, (img, dep, _, _) in enumerate(fr):
        ff.frame_upload(t, img, dep)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    return ff


def _plan(api, fr):
    return api.FusionFunctions.pack_replay(list(range(len(fr))), [f[3] for f in fr], np.stack([f[2] for f in fr]))


def _lockstep(api, cam, runs, want, tag, flags=0, fit_small_cap=None, constants=None):
    """the handles of `runs` as ONE batch, a frame at a time, every handle against its oracle after every frame; -> tier counts"""
    n = len(runs[0])
    handles, batch = [], None
    try:
        handles = [_handle(api, cam, fr, flags=flags, fit_small_cap=fit_small_cap, constants=constants) for fr in runs]
        plans = [_plan(api, fr) for fr in runs]
        batch = api.Batch(handles)
        tiers = []
        for t in range(n):
            s, r, p, m = api.Batch.pack([(pl[0][t:t + 1], pl[1][t:t + 1], pl[2][t:t + 1]) for pl in plans])
            batch.replay_enqueue(s, r, p, m)
            batch.synchronize()
            tiers += [h.debug_tier_counts() for h in handles]
            for b, h in enumerate(handles):
                _same_frame(f"{tag} handle {b} frame {t}", api, h, want[b][t])
        return tiers
    finally:
        if batch is not None:
            batch.close()
        for h in handles:
            h.close()


@pytest.fixture(scope="module")
def plain(mods):
    """camera name -> (camera, runs, oracle records): eight default scenes, four frames each, replayed once"""
    api, synth, ob = mods
    cache = {}

    def get(name, eigen33=False):
        if (name, eigen33) not in cache:
            cam = synth.TINY_RAGGED if name == "ragged" else F.tight_camera(synth)
            runs = cache[(name, False)][1] if (name, False) in cache else F.batch_runs(synth, cam)
            cache[(name, eigen33)] = (cam, runs, F.oracle_replays(ob, cam, runs, eigen33))
        return cache[(name, eigen33)]
    return get


# ---------------------------------------------------------------------------------------------------- 1. a batch of eight
@pytest.mark.parametrize("camera", ["ragged", "tight"])
def test_batch_of_eight(mods, plain, camera):
    api, synth, ob = mods
    cam, runs, want = plain(camera)
    S = (cam.width // 8) * (cam.height // 8)
    assert S % 64 != 0 and (cam.width % 64 == 0) == (camera == "tight")
    ff = _handle(api, cam, runs[0])
    try:
        assert ff.n_seed == S and ff.frame_pitch() == (cam.width + 63) // 64 * 64
    finally:
        ff.close()
    fitted = [int(F.has_plane(rec[2]).sum()) for rec in want[0]]
    assert min(fitted) > S // 6, fitted  # (the fit has work in every frame)
    tiers = _lockstep(api, cam, runs, want, camera)
    print(camera, "seeds with a plane per frame (handle 0)", fitted, "fit long groups max", max(tc["fit_long_groups"] for tc in tiers))


# ---------------------------------------------------------------------------------------------------- 2. the queue tier
def test_batch_of_eight_queue_tier(mods, plain):
    api, synth, ob = mods
    cam, runs, want = plain("ragged")
    tiers = _lockstep(api, cam, runs, want, "cap 0", fit_small_cap=0)
    # every group of four seeds with a list at all was queued for k_seed_fit<true, 2>, in every frame of every handle
    assert min(tc["fit_long_groups"] for tc in tiers) > 0, tiers
    print("fit long groups per frame and handle:", sorted({tc["fit_long_groups"] for tc in tiers}))


# ---------------------------------------------------------------------------------------------------- 3. planes come and go
HOLES = dict(hole_fraction=0.45, n_boxes=30)
# handle 0 (scene seed 40), frame t -> t + 1: a seed that has a plane in t and none in t + 1 / none in t and one in t + 1
LOSES = {0: 58, 1: 64, 2: 39}
GAINS = {0: 21, 1: 39, 2: 59}


def test_planes_come_and_go(mods):
    api, synth, ob = mods
    cam = synth.TINY_RAGGED
    runs = F.batch_runs(synth, cam, **HOLES)
    want = F.oracle_replays(ob, cam, runs)
    # the scene does what it was chosen for, on the host: both rules reject seeds in every frame, and between every pair of
    # frames the recorded seeds lose / gain their plane (a seed that loses it leaves its rows of the last fit behind)
    planes = []
    for t, (_, lab, seeds, _) in enumerate(want[0]):
        n, m, fitted = F.plane_census(lab, runs[0][t][1], seeds)
        assert np.array_equal(fitted, F.has_plane(seeds)), f"frame {t}: the census and the seed table disagree"
        assert ((n > 0) & (n < 16)).sum() >= 5 and ((n >= 16) & ~fitted).sum() >= 20, (t, n, fitted)
        planes.append(fitted)
    for t in range(len(planes) - 1):
        assert planes[t][LOSES[t]] and not planes[t + 1][LOSES[t]], (t, np.nonzero(planes[t] & ~planes[t + 1])[0].tolist())
        assert not planes[t][GAINS[t]] and planes[t + 1][GAINS[t]], (t, np.nonzero(~planes[t] & planes[t + 1])[0].tolist())
    _lockstep(api, cam, runs, want, "holes")
    _lockstep(api, cam, runs, want, "holes cap 0", fit_small_cap=0)


# ---------------------------------------------------------------------------------------------------- 4. groups against frames
@pytest.mark.parametrize("scene", ["plain", "holes"])
def test_frame_groups_of_four_against_single_frames(mods, plain, scene):
    api, synth, ob = mods
    if scene == "plain":
        cam, runs, want = plain("ragged")
        fr, recs = runs[0], want[0]
    else:
        cam = synth.TINY_RAGGED
        fr = F.batch_runs(synth, cam, **HOLES)[0]
        recs = F.oracle_replay(ob, cam, fr)
    assert len(fr) == 4
    state = {}
    for depth in (16, 1):  # 16: the superpixel stages of the four frames as one launch in the lane forms; 1: the wave forms
        ff = _handle(api, cam, fr, depth=depth)
        try:
            ff.replay_enqueue(*_plan(api, fr))
            ff.synchronize()
            _same_frame(f"{scene} depth {depth}", api, ff, recs[-1])
            state[depth] = (ff.labels(), ff.seeds(), ff.map_download())
        finally:
            ff.close()
    assert np.array_equal(state[16][0], state[1][0])
    assert fields_equal(state[16][1], state[1][1]) == [] and fields_equal(state[16][2], state[1][2]) == []


# ---------------------------------------------------------------------------------------------------- 5. the E33 variants
def test_batch_of_eight_eigen33(mods, plain):
    api, synth, ob = mods
    cam, runs, want = plain("ragged", eigen33=True)
    _lockstep(api, cam, runs, want, "eigen33", flags=api.DSM_FLAG_EIGEN33_PRODUCTS)
