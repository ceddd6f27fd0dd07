"""The crafted frames of tests/crafted_frames.py on the host:

  (a) the census: in PortOracle's state alone, every family puts seeds or pixels on both sides of the margin it is for;
  (b) where the reference translation unit has been built, it and PortOracle agree on every crafted frame fed twice -- labels,
      seed table and map, NaN == NaN (160x96 and the reference's own constants only: the reference has HUBER_RANGE compiled
      in, and at 166x103 it reads the record in front of its seed vector for the border pixels);
  (c) the host emulation of the device's formulation (tests/hostemu.cpp) reproduces the oracle on every crafted frame, with no
      violation of an error bound or of an exact-sum claim, and its counters say that the fit's branches are taken: residuals
      in all Huber classes at step 1, classes that change between steps, a non-empty class mask that stands (the cached
      inverse is reused after the mask comparison), an exactness test that fails (the ordered sums run)."""
import ctypes as C

import numpy as np
import pytest

import crafted_frames as cf
from conftest import fields_equal
from test_cpu import Emu

CASES = [(f, h) for f in cf.FAMILIES for h in (cf.HUBERS if f in cf.HUBER_FAMILIES else (0.4,))]
IDS = [f if f not in cf.HUBER_FAMILIES else f"{f}-{h}" for f, h in CASES]


@pytest.fixture(scope="module")
def ob(oracle_built):
    from oracle import bindings
    return bindings


@pytest.fixture(scope="module")
def synth():
    from densesurfelmapping_amd import synth
    return synth


def _same(tag, got, want):
    assert got[0] == want[0], f"{tag}: new surfel count {got[0]} vs {want[0]}"
    assert np.array_equal(got[1], want[1]), f"{tag}: {int((got[1] != want[1]).sum())} labels differ"
    assert fields_equal(got[2], want[2]) == [], f"{tag}: seed table differs {fields_equal(got[2], want[2])}"
    assert fields_equal(got[3], want[3]) == [], f"{tag}: map differs {fields_equal(got[3], want[3])}"


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("family,huber", CASES, ids=IDS)
def test_census(ob, synth, family, huber):
    cam = synth.TINY
    S = (cam.width // 8) * (cam.height // 8)
    assert S % 64 != 0  # (the last wave of the lane kernels is partial)
    cs = cf.check_census(ob, cam, family, huber)
    if family == "huber":
        assert min(c["lattice_cells"] for c in cs) >= cf.MEASURED["huber_lattice_cells"][huber] // 2
    if family == "edge":
        assert sum(c["on_float_below"] for c in cs) >= cf.MEASURED["edge_on_float_below"][huber] // 2
    if family == "lengths":
        assert max(c["longest_list"] for c in cs) == cf.MEASURED["longest_list"][(cam.width, cam.height)] == 64
    # the stage-by-stage replay the census reads IS the frame's state: the seed table of fuse_map on an empty map
    img, dep = cf.frames(ob, cam, family, huber)[0]
    rec = cf.replay(ob, cam, [(img, dep, cf.POSE, 0)], huber)[0]
    assert fields_equal(rec[2], cs[0]["post"]) == [] and np.array_equal(rec[1], cf.expected_labels(cam))


@pytest.mark.parametrize("family", ["valid", "lengths"])
def test_census_ragged(ob, synth, family):
    """166x103: the last cell column and row own the border pixels that have a candidate cell, so lists exceed 64"""
    cam = synth.TINY_RAGGED
    assert (cf.expected_labels(cam) < 0).any()  # (beyond them: pixels without a candidate cell, label -1)
    cs = cf.check_census(ob, cam, family)
    if family == "lengths":
        longest = max(c["longest_list"] for c in cs)
        assert longest == cf.MEASURED["longest_list"][(cam.width, cam.height)] and longest > 120  # (kFitSmallCap: the queue tier)


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("family", cf.FAMILIES)
def test_reference_agrees(ob, synth, family):
    if not ob.have_ref("serial"):
        return  # (the reference translation unit is built only where its sources are)
    cam = synth.TINY
    fr = cf.twice(cf.frames(ob, cam, family))
    for t, (got, want) in enumerate(zip(cf.replay(ob, cam, fr), cf.replay(ob, cam, fr, reference=True))):
        _same(f"{family} frame {t}", got, want)


# ---------------------------------------------------------------------------------------------------------------- (c)
def _emu_stats(emu, name, n):
    out = (C.c_longlong * n)()
    f = getattr(emu.lib, name)
    f.argtypes = [C.c_void_p, C.c_void_p]
    f(emu.h, out)
    return np.array(list(out), np.int64)


CLASS_STATS = ("first_noncore", "fitted", "seeds_mask_changed", "steps_mask_changed", "reuse_nonempty", "ordered_after_test")


def _emulate(ob, hostemu_lib, cam, family, huber):
    """the emulation through the family fed twice, every frame against the oracle; -> per frame the fit's counters"""
    fr = cf.twice(cf.frames(ob, cam, family, huber))
    want = cf.replay(ob, cam, fr, huber)
    emu = Emu(hostemu_lib, cam)
    emu.lib.emu_set_constants.argtypes = [C.c_void_p] + [C.c_double] * 4
    emu.lib.emu_set_constants(emu.h, huber, 0.5, 4.0, 0.1)
    le = np.zeros(0, ob.SURFEL_DTYPE)
    before, per_frame = _emu_stats(emu, "emu_fit_class_stats", 6), []
    for t, (img, dep, pose, ref) in enumerate(fr):
        le, ke = emu.fuse_map(ob.SURFEL_DTYPE, ref, img, dep, pose, le)
        _same(f"{family} {huber} frame {t}", (ke, emu.labels(), emu.seeds(ob.SEED_DTYPE), le), want[t])
        now = _emu_stats(emu, "emu_fit_class_stats", 6)
        per_frame.append(dict(zip(CLASS_STATS, (now - before).tolist())))
        before = now
    pick = _emu_stats(emu, "emu_fast_pick_stats", 24)
    assert pick[0] == len(fr) * 3 * cam.width * cam.height * np.mean(cf.expected_labels(cam) >= 0) and pick[3] > pick[0]
    assert pick[2] == 0 and pick[4] == 0, f"filtered pick: {pick[2]} other answers, {pick[4]} costs outside their bound"
    assert _emu_stats(emu, "emu_exact_sum_stats", 6)[3] == 0, "a qualifying sum differs in tree order"
    assert _emu_stats(emu, "emu_cert_stats", 3)[2] == 0, "sums that pass the exactness test differ from the ordered sums"
    emu.lib.emu_destroy(emu.h)
    return per_frame


@pytest.mark.parametrize("family,huber", CASES, ids=IDS)
def test_hostemu_reproduces_the_oracle(ob, synth, hostemu_lib, family, huber):
    per_frame = _emulate(ob, hostemu_lib, synth.TINY, family, huber)
    print(family, huber, per_frame[::2])
    if family == "classes":  # every frame of it is a far wall
        for t, st in enumerate(per_frame):
            assert st["first_noncore"] >= 60 and st["seeds_mask_changed"] >= 10, (t, st)
            assert st["first_noncore"] >= cf.MEASURED["first_noncore"] // 2, (t, st)
            assert st["seeds_mask_changed"] >= cf.MEASURED["seeds_mask_changed"] // 2, (t, st)
    if family == "huber" and huber == 0.05:
        for t, st in enumerate(per_frame):
            assert st["reuse_nonempty"] >= cf.MEASURED["reuse_nonempty"] // 2, (t, st)
    if family == "tiny":
        for t, st in enumerate(per_frame):
            assert st["ordered_after_test"] >= cf.MEASURED["ordered_after_test"] // 2, (t, st)


@pytest.mark.parametrize("family", ["valid", "lengths"])
def test_hostemu_reproduces_the_oracle_ragged(ob, synth, hostemu_lib, family):
    _emulate(ob, hostemu_lib, synth.TINY_RAGGED, family, 0.4)
