"""The painted frames of tests/painted_frames.py on the device: label images chosen pixel by pixel, so that superpixels of 1 to
225 pixels, depth lists on both sides of k_update_seeds' row limit, robust means of one to five passes, `moved` on the two
floats round 0.2, pixels that change owner in sweeps 1 and 2 and windows whose first depth decides the final labels reach
k_init_seeds(_lanes), k_assign, k_update_seeds, k_update_seeds_rest and k_update_seeds_wave on purpose.
Against PortOracle after every frame, every byte equal (NaN == NaN): new-surfel count, label image, seed table, map.  The
census of painted_frames.check_family is asserted first, on the oracle's state alone, and the lane forms must report EXACTLY
the census's queue lengths through dsm_debug_tier_counts: seeds queued for a wave of their own (list length >= 124 and no +inf
in it) and seeds queued for further Huber passes, per sweep.

  1. one handle, frame by frame (the wave-per-seed update, the 16-lane initialisation, k_assign<..., 1>): every family and
     variant fed twice, at 160x96 and 166x103; the tier counts stay zero;
  2. batches of eight handles (the lane forms), the families side by side in two arrangements.  A handle of a batch is fed
     its family's four variants one after the other (reference index 0 .. 3), not each frame twice: every frame is then
     fused into a map that ANOTHER label image made, the harder case; feeding a frame twice is case 1;
  3. frame groups of four (pipeline depth 8: the lane forms with lanes_from = 4): `lists`, `passes`, `drift` and `scan` as
     sequences of eight;
  4. 320x192: more than kRestOverBlocks = 128 seeds of one frame queued for a wave of their own, in a batch and in a group;
  5. fx != fy, and the RGB-D constant set, one batch each on the `sizes` family."""
import numpy as np
import pytest

import painted_frames as pf
from test_gpu_adversarial import _batched_lockstep, _check_final, _check_record, _gpu_record, _oracle_replays
from test_gpu_fit_masks import _handle, _plan
from test_gpu_parity import mods  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

ARRANGEMENTS = (("sizes", "lists", "lists_inf", "passes", "stable", "drift", "scan", "lists"),
                ("scan", "drift", "stable", "passes", "lists", "sizes", "lists_inf", "drift"))
IDENTITY = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def painted(mods):
    """censuses (checked) and oracle replays, each made once"""
    api, synth, ob = mods
    census, replays = {}, {}

    class Painted:
        def census(self, cam, family):
            """[variant] -> (n_over by sweep, n_rest by sweep)"""
            if (cam, family) not in census:
                _, seen = pf.check_family(ob, cam, family)
                census[(cam, family)] = [(i["n_over"], i["n_rest"]) for i in seen]
            return census[(cam, family)]

        def runs(self, cam, specs):
            """specs [(family, form, shift)] -> (runs, oracle replays as test_gpu_adversarial._oracle_replay makes them)"""
            missing = [sp for sp in specs if (cam, sp) not in replays]
            frames = []
            for family, form, shift in missing:
                self.census(cam, family)
                fr = pf.frames(cam, family)
                pose = IDENTITY if shift % 2 else pf.POSE
                frames.append({"twice": lambda: pf.twice(fr, pose), "lockstep": lambda: pf.lockstep(fr, shift, pose),
                               "eight": lambda: [(i, d, p, t) for t, (i, d, p, _) in enumerate(pf.lockstep(fr, shift, pose) * 2)]}[form]())
            for sp, fr, rep in zip(missing, frames, _oracle_replays(ob, cam, frames) if frames else []):
                replays[(cam, sp)] = (fr, rep)
            return [replays[(cam, sp)][0] for sp in specs], [replays[(cam, sp)][1] for sp in specs]

    return Painted()


def _tiers_equal(tag, tc, want):
    n_over, n_rest = want
    assert tc["long_list_by_sweep"] == n_over, f"{tag}: seeds queued for a wave of their own {tc['long_list_by_sweep']}, census {n_over}"
    assert tc["huber_rest_by_sweep"] == n_rest, f"{tag}: seeds queued for more Huber passes {tc['huber_rest_by_sweep']}, census {n_rest}"


# ------------------------------------------------------------------------------------------- 1. one handle, frame by frame
@pytest.mark.parametrize("camera", ["TINY", "TINY_RAGGED"])
@pytest.mark.parametrize("family", pf.FAMILIES)
def test_one_handle_frame_by_frame(mods, painted, family, camera):
    api, synth, ob = mods
    cam = getattr(synth, camera)
    (fr,), ((recs, orc, lo),) = painted.runs(cam, [(family, "twice", 0)])
    assert len(fr) == 2 * pf.VARIANTS
    ff = _handle(api, cam, fr)
    try:
        plan = _plan(api, fr)
        for t in range(len(fr)):
            ff.replay_enqueue(plan[0][t:t + 1], plan[1][t:t + 1], plan[2][t:t + 1])
            ff.synchronize()
            _check_record(f"{family} {camera} frame {t}", _gpu_record(ff), recs[t])
            tc = ff.debug_tier_counts()
            assert not any(tc["long_list_by_sweep"]) and not any(tc["huber_rest_by_sweep"]) and tc["fit_long_groups"] == 0, tc
        _check_final(f"{family} {camera}", api, ff, orc, lo)
    finally:
        ff.close()


# ------------------------------------------------------------------------------------------------- 2. batches of eight
def _batch(api, painted, cam, specs, tag):
    runs, want = painted.runs(cam, specs)
    tiers = _batched_lockstep(api, cam, runs, want, tag=tag)
    for t, per_handle in enumerate(tiers):
        for b, ((family, _, shift), tc) in enumerate(zip(specs, per_handle)):
            _tiers_equal(f"{tag} handle {b} ({family}) frame {t}", tc, painted.census(cam, family)[(t + shift) % pf.VARIANTS])
    return tiers


@pytest.mark.parametrize("camera", ["TINY", "TINY_RAGGED"])
@pytest.mark.parametrize("arrangement", [0, 1])
def test_batch_of_eight(mods, painted, arrangement, camera):
    api, synth, ob = mods
    cam = getattr(synth, camera)
    specs = [(f, "lockstep", (b + arrangement) % pf.VARIANTS) for b, f in enumerate(ARRANGEMENTS[arrangement])]
    assert len(specs) == 8 and set(ARRANGEMENTS[arrangement]) == set(pf.FAMILIES)
    tiers = _batch(api, painted, cam, specs, f"{camera} arrangement {arrangement}")
    print(camera, arrangement, "queued for a wave / for more passes, frame 0:",
          [(tc["long_list_by_sweep"], tc["huber_rest_by_sweep"]) for tc in tiers[0]])


# ---------------------------------------------------------------------------------------------- 3. frame groups of four
def _groups(api, painted, cam, family, tag):
    (fr,), ((recs, orc, lo),) = painted.runs(cam, [(family, "eight", 0)])
    assert len(fr) == 8
    ff = api.FusionFunctions.from_camera(cam, frame_slots=8, surfel_capacity=1 << 20, pipeline_depth=8)
    try:
        for t, (img, dep, _, _) in enumerate(fr):
            ff.frame_upload(t, img, dep)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        slots, refs, poses = _plan(api, fr)
        for g in (0, 4):
            ff.replay_enqueue(slots[g:g + 4], refs[g:g + 4], poses[g:g + 4])
            tc = ff.debug_tier_counts()  # (the latest frame's: the last of the group)
            _check_record(f"{tag} frame {g + 3}", _gpu_record(ff), recs[g + 3])
            _tiers_equal(f"{tag} frame {g + 3}", tc, painted.census(cam, family)[3])
        _check_final(tag, api, ff, orc, lo)
    finally:
        ff.close()


@pytest.mark.parametrize("camera", ["TINY", "TINY_RAGGED"])
@pytest.mark.parametrize("family", ["lists", "passes", "drift", "scan"])
def test_frame_groups_of_four(mods, painted, family, camera):
    api, synth, ob = mods
    _groups(api, painted, getattr(synth, camera), family, f"{family} {camera} groups")


# ---------------------------------------------------------------------------------------- 4. past the over-block count
def test_past_the_over_blocks_batch(mods, painted):
    api, synth, ob = mods
    cam = pf.wide_camera(synth)
    assert min(n_over[0] for n_over, _ in painted.census(cam, "lists_long")) >= 200 > 128  # (kRestOverBlocks)
    _batch(api, painted, cam, [("lists_long", "lockstep", b % pf.VARIANTS) for b in range(8)], "320x192")


def test_past_the_over_blocks_group(mods, painted):
    api, synth, ob = mods
    cam = pf.wide_camera(synth)
    assert min(n_over[0] for n_over, _ in painted.census(cam, "lists_long")) >= 200 > 128
    _groups(api, painted, cam, "lists_long", "320x192 groups")


# ------------------------------------------------------------------------------- 5. fx != fy, the RGB-D constant set
@pytest.mark.parametrize("kind", ["fx_ne_fy", "rgbd"])
def test_batch_of_eight_other_cameras(mods, painted, kind):
    api, synth, ob = mods
    T = synth.TINY
    cam = (synth.Camera(T.width, T.height, 117.3, 123.9, T.cx, T.cy) if kind == "fx_ne_fy"
           else synth.Camera(T.width, T.height, T.fx, T.fy, T.cx, T.cy, far=6.0, near=0.3, rgbd=True))
    _batch(api, painted, cam, [("sizes", "lockstep", b % pf.VARIANTS) for b in range(8)], kind)
