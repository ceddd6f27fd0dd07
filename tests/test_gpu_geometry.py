"""The frame path on the device at the image sizes of tests/geometry_cases.py: tile edges of k_assign and k_pixel_normals, grids
three cells thin, seed counts on either side of a wave, of a workgroup and of every S mod 4, sides of 32767 pixels, labels with
bit 15 set and the top label 65534.  One test id per (geometry, form), small sizes first; every id compares the new-surfel count,
the label image, the seed table and the surfel array with PortOracle after the frames named below, every byte equal, NaN == NaN
(that the oracle's replay is worth comparing with -- the census -- and that the reference agrees with it at these sizes is
tests/test_cpu_geometry.py's business).

  dropin, resident  one handle, frame by frame: the wave-per-seed forms (k_init_seeds, k_assign<.., 1>, k_update_seeds_wave,
                    k_seed_points, k_seed_fit<false, kFitAll>), through fuse_map and through frame_upload + fuse_frame_resident;
                    checked after every frame
  batch8, batch8-cap0
                    eight handles in lockstep, each its own variant of the frames: the lane-per-seed forms (k_init_seeds_lanes,
                    k_assign<.., 4>, k_update_seeds + _rest, k_pixel_normals + k_seed_stats, both fit tiers), the short tier's
                    limit as shipped and at 0; checked after every frame
  groups            one sequence at pipeline depth 8 (frame groups of four in the lane forms), six frames: the group, then the
                    ragged end frame by frame; checked after the group and at the end.  The four sizes above half a megapixel,
                    whose other runs have two frames, take five here.

What each id asserts about the form that ran: dsm_debug_tier_counts is zero throughout after a wave-form frame (only
k_update_seeds queues seeds, only a batched fit counts long groups); after a lane-form frame some seed was queued for another
Huber pass, and with the limit at 0 every fitted group of four is a long group."""
import numpy as np
import pytest

import geometry_cases as gc
from test_gpu_adversarial import _batched_lockstep, _check_final, _check_record, _gpu_record, _oracle_replays
from test_gpu_parity import mods  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

FORMS = ("dropin", "resident", "batch8", "batch8-cap0", "groups")
CASES = [(g.name, f) for g in gc.GEOMETRIES for f in FORMS]


@pytest.fixture(scope="module")
def replays(mods):
    """geometry, number of variants[, frames per run] -> (runs, oracle replays) of the first variants, made once; only the
    latest geometry and run length are kept (the ids come geometry by geometry, and eight oracles at four megapixels are a
    gigabyte)"""
    api, synth, ob = mods
    held = {}

    def get(g, n_variants, n_frames=None):
        n_frames = n_frames or g.n_frames
        if held.get("key") != (g.name, n_frames):
            held.clear()
            held.update(key=(g.name, n_frames), runs=[], want=[])
        have = len(held["runs"])
        if have < n_variants:
            more = [gc.frames(g, n_frames, v) for v in range(have, n_variants)]
            held["runs"] += more
            held["want"] += _oracle_replays(ob, g.camera, more)
        return held["runs"][:n_variants], held["want"][:n_variants]
    return get


def _no_lane_form_ran(tag, tc):
    assert not any(tc["huber_rest_by_sweep"]) and not any(tc["long_list_by_sweep"]) and tc["fit_long_groups"] == 0, (tag, tc)


def _one_handle(api, g, fr, want, resident):
    recs, orc, lo = want
    ff = api.FusionFunctions.from_camera(g.camera, frame_slots=len(fr), surfel_capacity=1 << 18)
    try:
        assert ff.n_seed == g.S
        lg = np.zeros(0, api.SURFEL_DTYPE)
        if resident:
            for t, (img, dep, _, _) in enumerate(fr):
                ff.frame_upload(t, img, dep)
            ff.map_upload(lg)
        for t, (img, dep, pose, ref) in enumerate(fr):
            tag = f"{g.name} {'resident' if resident else 'dropin'} frame {t}"
            if resident:
                ff.fuse_frame_resident(t, ref, pose)
                ff.synchronize()
            else:
                lg, k = ff.fuse_map(ref, img, dep, pose, lg)
                assert (k, len(lg)) == recs[t][:2], f"{tag}: {(k, len(lg))} new / live surfels, the oracle {recs[t][:2]}"
            _check_record(tag, _gpu_record(ff), recs[t])
            _no_lane_form_ran(tag, ff.debug_tier_counts())
        _check_final(f"{g.name} after {len(fr)} frames", api, ff, orc, lo)
    finally:
        ff.close()


def _batch_of_eight(api, g, runs, want, cap):
    tiers = _batched_lockstep(api, g.camera, runs, want, cap, tag=f"{g.name} cap {cap}")
    flat = [tc for per_frame in tiers for tc in per_frame]
    rest, long_groups = max(max(tc["huber_rest_by_sweep"]) for tc in flat), max(tc["fit_long_groups"] for tc in flat)
    print(g.name, "cap", cap, "huber rest max", rest, "long lists", sum(sum(tc["long_list_by_sweep"]) for tc in flat), "fit long groups max", long_groups)
    # the lane forms ran: only k_update_seeds queues seeds for more Huber passes.  Every geometry's frames have a step edge and
    # holes under some seed, nine seeds included
    assert rest > 0, flat
    assert long_groups <= (g.S + 3) // 4
    if cap == 0:  # every group with a fitted seed goes to the full-length tier, and every frame of every run fits seeds
        assert all(tc["fit_long_groups"] > 0 for tc in flat), flat


def _frame_groups(api, g, fr, want):
    recs, orc, lo = want
    n, G = len(fr), 4
    grouped = n - n % G
    assert n == g.group_frames and grouped == 4 and g.quiet_frame < grouped < n
    ff = api.FusionFunctions.from_camera(g.camera, frame_slots=n, surfel_capacity=1 << 18, pipeline_depth=8)
    try:
        for t, (img, dep, _, _) in enumerate(fr):
            ff.frame_upload(t, img, dep)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        slots, refs, poses = api.FusionFunctions.pack_replay(list(range(n)), [f[3] for f in fr], np.stack([f[2] for f in fr]))
        ff.replay_enqueue(slots[:grouped], refs[:grouped], poses[:grouped])
        ff.synchronize()
        tc = ff.debug_tier_counts()  # (the latest frame's: the last of the group)
        print(g.name, "group of four, last frame:", tc)
        _check_record(f"{g.name} groups frame {grouped - 1}", _gpu_record(ff), recs[grouped - 1])
        assert any(tc["huber_rest_by_sweep"]), (g.name, tc)  # (the lane forms: see _batch_of_eight)
        ff.replay_enqueue(slots[grouped:], refs[grouped:], poses[grouped:])
        ff.synchronize()
        _check_record(f"{g.name} groups frame {n - 1}", _gpu_record(ff), recs[n - 1])
        _no_lane_form_ran(f"{g.name} groups, ragged end", ff.debug_tier_counts())  # (frame by frame: the wave forms again)
        _check_final(f"{g.name} groups after {n} frames", api, ff, orc, lo)
    finally:
        ff.close()


@pytest.mark.parametrize("name,form", CASES, ids=[f"{n}-{f}" for n, f in CASES])
def test_geometry(mods, replays, name, form):
    api, synth, ob = mods
    g = gc.BY_NAME[name]
    if form in ("dropin", "resident"):
        runs, want = replays(g, 1)
        _one_handle(api, g, runs[0], want[0], resident=form == "resident")
    elif form == "groups":
        runs, want = replays(g, 1, g.group_frames)
        _frame_groups(api, g, runs[0], want[0])
    else:
        runs, want = replays(g, gc.VARIANTS)
        _batch_of_eight(api, g, runs, want, 0 if form == "batch8-cap0" else None)


def test_sizes_at_the_acceptance_bounds(mods):
    """dsm_create's size check on either side of its two bounds: 65535 superpixels (test_api_errors_are_reported has 3840x2160)
    and three cells per side"""
    api, synth, ob = mods
    ff = api.FusionFunctions().initialize(2040, 2056, 1800.0, 1900.0, 1000.0, 1100.0, 30, 0.5, surfel_capacity=1024)  # 255 x 257 = 65535
    assert ff.n_seed == 65535
    ff.close()
    with pytest.raises(api.DsmError) as ei:  # 256 x 257 = 65792
        api.FusionFunctions().initialize(2048, 2056, 1800.0, 1900.0, 1000.0, 1100.0, 30, 0.5, surfel_capacity=1024)
    assert ei.value.code == -1 and "65535 superpixels" in str(ei.value)
    ff = api.FusionFunctions().initialize(24, 24, 20.0, 21.0, 11.0, 12.0, 30, 0.5, surfel_capacity=1024)
    assert ff.n_seed == 9
    ff.close()
    for w, h in ((23, 24), (24, 23)):
        with pytest.raises(api.DsmError) as ei:
            api.FusionFunctions().initialize(w, h, 20.0, 21.0, 11.0, 12.0, 30, 0.5, surfel_capacity=1024)
        assert ei.value.code == -1, (w, h)
