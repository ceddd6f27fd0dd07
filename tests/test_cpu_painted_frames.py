"""The painted frames of tests/painted_frames.py on the host:

  (a) the census: PortOracle's labels after every sweep ARE the painted design, the numpy restatement of update_seeds equals
      the oracle's seed table bit for bit, and every family puts its seeds where it says (sizes, list lengths on both sides of
      124, pass counts 1 .. 5, moved on both sides of 0.2, pixels that change owner in sweeps 1 and 2, a seed initialisation whose
      scan order shows in the final labels) -- at 160x96 and 166x103, with the figures MEASURED records;
  (b) where the reference translation unit has been built, it and PortOracle agree on every painted frame fed twice (160x96
      only: at 166x103 the reference reads the record in front of its seed vector for the border pixels);
  (c) the host emulation of the device's formulation (tests/hostemu.cpp) reproduces the oracle on every painted frame fed twice
      -- labels, seed table, map -- with no pick_seed_fast bound violated and no fast pick answered differently; the pixels the
      fp32 filter left open are printed per family (painted frames are full of equal-intensity ties)."""
import numpy as np
import pytest

import crafted_frames as cf
import painted_frames as pf
from test_cpu import Emu
from test_cpu_crafted_frames import _emu_stats, _same

CAMERAS = ("TINY", "TINY_RAGGED")


@pytest.fixture(scope="module")
def ob(oracle_built):
    from oracle import bindings
    return bindings


@pytest.fixture(scope="module")
def synth():
    from densesurfelmapping_amd import synth
    return synth


def _replay(ob, cam, fr, reference=False):
    return cf.replay(ob, cam, fr, reference=reference)


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("family", pf.FAMILIES)
def test_census(ob, synth, family, camera):
    cam = getattr(synth, camera)
    cs, seen = pf.check_family(ob, cam, family)
    size = (cam.width, cam.height)
    for v, info in enumerate(seen):
        print(family, size, v, info)
        assert info["n_over"] == pf.MEASURED[family][size]["n_over"][v], (family, size, v, info["n_over"])
        assert info["n_rest"] == pf.MEASURED[family][size]["n_rest"][v], (family, size, v, info["n_rest"])
        assert 0 < info["stable_after"][0] < len(cs[v][0]["cnt"])  # (sweep 1 skips some seeds and recomputes others)
    if family == "stable":
        for key in ("at_or_above", "below", "on_float_0.2", "on_float_below", "by_centroid", "probes_left", "probes_kept", "probes_left_on_float_0.2"):
            assert [i[key] for i in seen] == pf.MEASURED["stable"][size][key], (key, [i[key] for i in seen])
    if family == "scan":
        for key in ("crafted", "changed_by_reversal", "no_depth_at_all", "kinds", "pairs_changed_by_swap", "row15_changed_by_stopping_early",
                    "earlier_row_later_column", "first_in_tell_tale_row", "first_in_column_15", "clipped_left_or_top",
                    "last_column_unseen", "last_row_unseen"):
            assert [i[key] for i in seen] == pf.MEASURED["scan"][size][key], (key, [i[key] for i in seen])
        assert min(i["share"] for i in seen) >= 0.8
    if family == "lists":
        assert [i["placements"] for i in seen] == pf.MEASURED["lists"][size]["placements"]
    if family == "drift":
        for key in ("changed", "old_seed_stable"):
            assert [i[key] for i in seen] == pf.MEASURED["drift"][size][key], (key, [i[key] for i in seen])
        assert min(i["n_over"][2] for i in seen) > 0 and min(i["n_rest"][2] for i in seen) > 0  # (sweep 2 has work in both queues)
    if family == "passes":
        assert [i["per_pass_count"] for i in seen] == pf.MEASURED["passes"][size]["per_pass_count"]
    # the stage-by-stage replay the census reads IS the frame's superpixel state: labels of fuse_map on an empty map
    img, dep, owner = pf.frames(cam, family)[0]
    rec = _replay(ob, cam, [(img, dep, pf.POSE, 0)])[0]
    assert np.array_equal(rec[1], owner[-1] if isinstance(owner, list) else owner)


def test_census_past_the_over_blocks(ob, synth):
    cam = pf.wide_camera(synth)
    cs, seen = pf.check_family(ob, cam, "lists_long")
    print("lists_long", [i["n_over"] for i in seen])
    assert min(i["n_over"][0] for i in seen) >= 200 > 128  # (kRestOverBlocks)
    assert [i["n_over"] for i in seen] == pf.MEASURED["lists_long"]["n_over"]


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("family", pf.FAMILIES)
def test_reference_agrees(ob, synth, family):
    if not ob.have_ref("serial"):
        return  # (the reference translation unit is built only where its sources are)
    cam = synth.TINY
    fr = pf.twice(pf.frames(cam, family))
    for t, (got, want) in enumerate(zip(_replay(ob, cam, fr), _replay(ob, cam, fr, reference=True))):
        _same(f"{family} frame {t}", got, want)


# ---------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("family", pf.FAMILIES)
def test_hostemu_reproduces_the_oracle(ob, synth, hostemu_lib, family, camera):
    cam = getattr(synth, camera)
    fr = pf.twice(pf.frames(cam, family))
    want = _replay(ob, cam, fr)
    emu = Emu(hostemu_lib, cam)
    le = np.zeros(0, ob.SURFEL_DTYPE)
    try:
        for t, (img, dep, pose, ref) in enumerate(fr):
            le, ke = emu.fuse_map(ob.SURFEL_DTYPE, ref, img, dep, pose, le)
            _same(f"{family} {camera} frame {t}", (ke, emu.labels(), emu.seeds(ob.SEED_DTYPE), le), want[t])
        pick = _emu_stats(emu, "emu_fast_pick_stats", 24)
    finally:
        emu.lib.emu_destroy(emu.h)
    print(family, camera, "pixels picked", int(pick[0]), "left open by the fp32 filter", int(pick[1]), "costs checked", int(pick[3]))
    assert pick[0] > 0 and pick[3] > 0
    assert pick[2] == 0 and pick[4] == 0, f"filtered pick: {pick[2]} other answers, {pick[4]} costs outside their bound"
    assert int(pick[1]) == pf.MEASURED[family][(cam.width, cam.height)]["pick_left_open"], int(pick[1])
