"""The crafted frames of tests/crafted_frames.py on the device: depth images whose pixels sit on the decision margins of
k_pixel_normals, k_seed_points / k_seed_stats, k_seed_fit (all three tiers), k_seed_finish, k_frame_tail and the robust mean
of k_update_seeds.  Against PortOracle after every frame, every byte equal (NaN == NaN): new-surfel count, label image,
seed table, map.  The census of crafted_frames.check_census is asserted first, on the oracle's state alone, so that a
comparison that passes has compared what the frames were built for.

  1. one handle, frame by frame (the wave forms, k_seed_points): every variant of every family fed twice, so that
     k_fuse_surfels meets the planes the frame made;
  2. a batch of eight handles, one family per handle, the four variants in lockstep (the lane forms);
  3. that batch with the short tier's limit at 0, at the longest inlier list the census found and at one less: the tier
     boundary `m_max > fit_small_cap` on a length that occurs;
  4. one handle at pipeline depth 16 (a frame group of four: the lane forms with masks) against the same handle at depth 1;
  5. the batch with DSM_FLAG_EIGEN33_PRODUCTS;
  6. 166x103: the last cell column and row own the border pixels, lists run to 144 and the queue tier takes them unasked."""
import numpy as np
import pytest

import crafted_frames as cf
from conftest import fields_equal
from test_gpu_fit_masks import _handle, _lockstep, _plan, _same_frame
from test_gpu_parity import mods  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

CASES = [(f, h) for f in cf.FAMILIES for h in (cf.HUBERS if f in cf.HUBER_FAMILIES else (0.4,))]
IDS = [f if f not in cf.HUBER_FAMILIES else f"{f}-{h}" for f, h in CASES]


@pytest.fixture(scope="module")
def crafted(mods):
    """(camera name, family, huber) -> the censuses of the four variants, checked; and the oracle's replays, each made once"""
    api, synth, ob = mods
    census, replays = {}, {}

    class Crafted:
        @staticmethod
        def cam(name):
            return synth.TINY_RAGGED if name == "ragged" else synth.TINY

        def census(self, family, huber=0.4, name="tiny"):
            key = (name, family, huber if family in cf.HUBER_FAMILIES else 0.4)
            if key not in census:
                census[key] = cf.check_census(ob, self.cam(name), family, huber)
            return census[key]

        def frames(self, family, huber=0.4, name="tiny"):
            self.census(family, huber, name)
            return cf.frames(ob, self.cam(name), family, huber)

        def replay(self, form, family, huber=0.4, name="tiny", eigen33=False, shift=0):
            """form: cf.twice or cf.lockstep; shift: the variants rotated (handles of one family that differ)"""
            key = (form.__name__, name, family, huber, eigen33, shift)
            if key not in replays:
                fr = self.frames(family, huber, name)
                fr = form(fr[shift:] + fr[:shift])
                replays[key] = (fr, cf.replay(ob, self.cam(name), fr, huber, eigen33))
            return replays[key]

    return Crafted()


def _fitted(rec):
    return int(cf.has_plane(rec[2]).sum())


# ------------------------------------------------------------------------------------------- 1. one handle, frame by frame
@pytest.mark.parametrize("family,huber", CASES, ids=IDS)
def test_one_handle_frame_by_frame(mods, crafted, family, huber):
    api, synth, ob = mods
    cam = synth.TINY
    fr, want = crafted.replay(cf.twice, family, huber)
    assert len(fr) == 2 * cf.VARIANTS
    ff = _handle(api, cam, fr, constants=cf.constants_of(huber))
    try:
        plan = _plan(api, fr)
        for t in range(len(fr)):
            ff.replay_enqueue(plan[0][t:t + 1], plan[1][t:t + 1], plan[2][t:t + 1])
            ff.synchronize()
            _same_frame(f"{family} {huber} frame {t}", api, ff, want[t])
    finally:
        ff.close()


# ------------------------------------------------------------------------------------------------- 2. a batch of eight
def _batch(crafted, huber, second, eigen33=False):
    fams = cf.batch_families(second)
    pairs = [crafted.replay(cf.lockstep, f, huber, eigen33=eigen33) for f in fams]
    return fams, [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("huber,second", [(0.4, False), (0.4, True), (0.05, True), (0.5, True)],
                         ids=["0.4-walls", "0.4-edge-tiny", "0.05-edge-tiny", "0.5-edge-tiny"])
def test_batch_of_eight(mods, crafted, huber, second):
    api, synth, ob = mods
    fams, runs, want = _batch(crafted, huber, second)
    assert len(runs) == 8 and all(len(r) == 4 for r in runs)
    _lockstep(api, synth.TINY, runs, want, f"batch {huber} {fams}", constants=cf.constants_of(huber))


# ------------------------------------------------------------------------------------------------ 3. the tier boundary
@pytest.mark.parametrize("cap", ["zero", "longest", "one_less"])
def test_batch_of_eight_at_the_tier_boundary(mods, crafted, cap):
    api, synth, ob = mods
    fams, runs, want = _batch(crafted, 0.4, False)
    longest = max(c["longest_list"] for f in fams for c in crafted.census(f))
    assert longest == cf.MEASURED["longest_list"][(160, 96)]
    tiers = _lockstep(api, synth.TINY, runs, want, f"cap {cap}", fit_small_cap={"zero": 0, "longest": longest, "one_less": longest - 1}[cap])
    groups = np.array([tc["fit_long_groups"] for tc in tiers]).reshape(4, 8)  # [frame, handle]
    fitted = np.array([[_fitted(want[b][t]) for b in range(8)] for t in range(4)])
    print(f"cap {cap}: fit long groups per frame and handle\n{groups}")
    if cap == "longest":
        assert (groups == 0).all(), groups
    elif cap == "one_less":
        assert groups.max() > 0, groups
        assert (groups[:, fams.index("wall001")] == 0).all()
    else:
        assert ((groups > 0) == (fitted > 0)).all(), (groups, fitted)
        assert (fitted > 0).sum() >= 28  # (every frame of seven families has fitted seeds)


# ---------------------------------------------------------------------------------------- 4. groups against frames
@pytest.mark.parametrize("family,huber", CASES, ids=IDS)
def test_frame_group_of_four_against_single_frames(mods, crafted, family, huber):
    api, synth, ob = mods
    fr, want = crafted.replay(cf.lockstep, family, huber)
    assert len(fr) == 4
    state = {}
    for depth in (16, 1):  # 16: the superpixel stages of the four frames as one launch in the lane forms; 1: the wave forms
        ff = _handle(api, synth.TINY, fr, depth=depth, constants=cf.constants_of(huber))
        try:
            ff.replay_enqueue(*_plan(api, fr))
            ff.synchronize()
            _same_frame(f"{family} {huber} depth {depth}", api, ff, want[-1])
            state[depth] = (ff.labels(), ff.seeds(), ff.map_download())
        finally:
            ff.close()
    assert np.array_equal(state[16][0], state[1][0])
    assert fields_equal(state[16][1], state[1][1]) == [] and fields_equal(state[16][2], state[1][2]) == []


# ------------------------------------------------------------------------------------------------ 5. the E33 variants
def test_batch_of_eight_eigen33(mods, crafted):
    api, synth, ob = mods
    fams, runs, want = _batch(crafted, 0.4, False, eigen33=True)
    plain = _batch(crafted, 0.4, False)[2]
    moved = sum(fields_equal(a[3], b[3]) != [] for wa, wb in zip(want, plain) for a, b in zip(wa, wb) if len(a[3]) == len(b[3]))
    assert moved > 0, "the flag moves no surfel of the crafted frames: it would not be exercised"
    _lockstep(api, synth.TINY, runs, want, "eigen33", flags=api.DSM_FLAG_EIGEN33_PRODUCTS)


# --------------------------------------------------------------------------------------------------- 6. the ragged camera
def test_batch_of_eight_ragged(mods, crafted):
    api, synth, ob = mods
    cam = synth.TINY_RAGGED
    cs = crafted.census("lengths", name="ragged")
    crafted.census("valid", name="ragged")
    longest = max(c["longest_list"] for c in cs)
    assert longest == cf.MEASURED["longest_list"][(166, 103)] and longest > 120  # (past kFitSmallCap: the queue tier, unasked)
    pairs = [crafted.replay(cf.lockstep, f, name="ragged", shift=b // 2) for b, f in enumerate(("valid", "lengths") * 4)]
    tiers = _lockstep(api, cam, [p[0] for p in pairs], [p[1] for p in pairs], "ragged")
    groups = np.array([tc["fit_long_groups"] for tc in tiers]).reshape(4, 8)
    print(f"ragged: fit long groups per frame and handle\n{groups}")
    # the list-length handles queue the corner cell's group where its list is 144, 121 or 143 long and not where it is 120, the
    # short tier's limit itself (handle b sees the variants rotated by b // 2); the valid-count handles, whose lists end at 18, none
    for b in range(8):
        for t in range(4):
            longest = cs[(t + b // 2) % 4]["longest_list"]
            assert longest == cf.CORNER_LENGTHS[(t + b // 2) % 4]
            assert groups[t, b] == (1 if b % 2 and longest > 120 else 0), (t, b, groups)
