"""Device parity on crafted maps (tests/crafted_maps.py): every exit of k_fuse_surfels at its margin, fx != fy, caller-chosen
constants and the double form of the depth tolerance, through every form of the fuse path -- drop-in (eager and graph),
resident, the drop-in's delta download, batches of eight, frame groups, DSM_FLAG_EIGEN33_PRODUCTS and uint16 depth.

Every comparison is with PortOracle on identical input: map, label image and seed table (its `fused` marks included) equal
byte for byte, NaN == NaN, and the new-surfel counts equal.  tests/test_cpu_crafted_maps.py guards the inputs: it counts, in
the oracle's result, that every group of records takes the exit it was built for.
"""
import numpy as np
import pytest

import crafted_maps as cm
from conftest import fields_equal
from test_gpu_parity import _compare_frame

pytestmark = pytest.mark.gpu

IDS = list(cm.CASES)
LENGTHS = (1, 63, 64, 65, 255, 256, 257, None)  # None: the whole map


@pytest.fixture(scope="module")
def mods(oracle_built):
    import torch
    torch.cuda.init()  # torch's lazy HIP initialisation first, as in the other GPU suites
    from densesurfelmapping_amd import api, synth
    from oracle import bindings
    return api, synth, bindings


_CASES = {}


def _case(cid, seed=1, u16_scale=None):
    """make_case's tuple for a CASES id, built once per (id, seed)"""
    key = (cid, seed, u16_scale)
    if key not in _CASES:
        cam, k, _ = cm.CASES[cid]
        _CASES[key] = cm.make_case(cam, k, seed, u16_scale=u16_scale)
    return _CASES[key]


def _pair(mods, cid, flags=0, eigen33=False, **kw):
    api, synth, ob = mods
    cam, k, _ = cm.CASES[cid]
    kw.setdefault("surfel_capacity", 1 << 14)
    if eigen33:
        flags |= api.DSM_FLAG_EIGEN33_PRODUCTS
    ff = api.FusionFunctions.from_camera(cam, flags=flags, constants=cm.constants_arg(cam, k), **kw)
    return ff, ob.PortOracle(cam, constants=k, eigen33=eigen33)


def _dropin_two_frames(mods, cid, flags=0, eigen33=False):
    """the crafted frame over the crafted map, then the scene's next frame over the result; returns the map after the first"""
    api, synth, ob = mods
    cam = cm.CASES[cid][0]
    img, dep, pose, ref, surfels, _ = _case(cid)
    ff, orc = _pair(mods, cid, flags, eigen33)
    try:
        lg, kg = ff.fuse_map(ref, img, dep, pose, surfels.astype(api.SURFEL_DTYPE))
        lo, ko = orc.fuse_map(ref, img, dep, pose, surfels)
        assert kg == ko, f"{cid}: new surfel count {kg} vs {ko}"
        _compare_frame(f"{cid} crafted frame", ff, orc, lg, lo.astype(api.SURFEL_DTYPE))
        first = lg
        img2, dep2, pose2 = cm.second_frame(cam, 1)
        lg, kg = ff.fuse_map(ref + 1, img2, dep2, pose2, lg)
        lo, ko = orc.fuse_map(ref + 1, img2, dep2, pose2, lo)
        assert kg == ko, f"{cid}: second frame, new surfel count {kg} vs {ko}"
        assert len(lg) < len(first), "the second frame was to shrink the map"
        _compare_frame(f"{cid} second frame", ff, orc, lg, lo.astype(api.SURFEL_DTYPE))
        return first
    finally:
        ff.close()


@pytest.mark.parametrize("flags", [1, 0], ids=["eager", "graph"])
@pytest.mark.parametrize("cid", IDS)
def test_dropin(mods, cid, flags):
    """dsm_fuse_map handed a caller's crafted vector, then a second frame on the compacted result"""
    _dropin_two_frames(mods, cid, flags)


@pytest.mark.parametrize("cid", ["default", "double_scale"])
def test_map_length_edges(mods, cid):
    """the crafted map cut to 1, 63, 64, 65, 255, 256, 257 records and whole, its last record in turn one that fuses, one
    that is deleted and a hole: the ragged last vector of records_land / records_from_lds, the last word of the hole bitmap"""
    api, synth, ob = mods
    img, dep, pose, ref, surfels, _ = _case(cid)
    ff, orc = _pair(mods, cid)
    try:
        after, _ = orc.fuse_initialize_map(ref, img, dep, pose, surfels)
        outcome = cm.outcomes(surfels, after)
        for n in LENGTHS:
            for last in ("fused", "deleted", "hole"):
                m = cm.cut(surfels, outcome, n or len(surfels), last)
                lg, kg = ff.fuse_map(ref, img, dep, pose, m.astype(api.SURFEL_DTYPE))
                lo, ko = orc.fuse_map(ref, img, dep, pose, m)
                assert kg == ko, (cid, n, last, kg, ko)
                _compare_frame(f"{cid} length {n} ending in a {last}", ff, orc, lg, lo.astype(api.SURFEL_DTYPE))
    finally:
        ff.close()


@pytest.mark.parametrize("cid", IDS)
def test_resident_and_delta_download(mods, cid):
    """map_upload + frame_upload + fuse_frame_resident + map_download; then the drop-in on the caller's own array, where the
    second and third call bring back only the 64-record groups the frame changed: waves without a change, a shrinking map"""
    api, synth, ob = mods
    cam = cm.CASES[cid][0]
    img, dep, pose, ref, surfels, intent = _case(cid)
    ff, orc = _pair(mods, cid, frame_slots=2)
    try:
        ff.map_upload(surfels.astype(api.SURFEL_DTYPE))
        ff.frame_upload(0, img, dep)
        ff.fuse_frame_resident(0, ref, pose)
        ff.synchronize()
        lo, ko = orc.fuse_map(ref, img, dep, pose, surfels)
        assert ff.last_new_count() == ko
        _compare_frame(f"{cid} resident", ff, orc, ff.map_download(), lo.astype(api.SURFEL_DTYPE))
        # the caller's array through three calls: the crafted frame (whole map up and down), the crafted frame once more
        # (a delta: the records that fused fuse again, the rest stands), the next frame (a delta on a shrinking map)
        # (behind the crafted records, forty waves that no frame touches: the delta path is taken while fewer than six
        # tenths of the map's groups change)
        mine = np.concatenate([surfels, np.tile(surfels[intent == "parked"], 40)])
        buf = np.zeros(len(mine) + 3 * ff.n_seed, api.SURFEL_DTYPE)
        buf[:len(mine)] = mine
        n, lo = len(mine), mine
        img2, dep2, pose2 = cm.second_frame(cam, 1)
        before = ff.debug_dropin_stats()
        for call, (r, i, d, p) in enumerate(((ref, img, dep, pose), (ref + 1, img, dep, pose), (ref + 2, img2, dep2, pose2))):
            n_in = n
            n, k = ff.fuse_map_inplace(r, i, d, p, buf, n)
            lo, ko = orc.fuse_map(r, i, d, p, lo)
            assert k == ko and n == len(lo), (cid, call, k, ko, n, len(lo))
            assert fields_equal(buf[:n], lo.astype(api.SURFEL_DTYPE)) == [], (cid, call)
        after = ff.debug_dropin_stats()
        assert n < n_in, "the last call was to shrink the map"
        assert after["delta_calls"] - before["delta_calls"] >= 1, ("no call took the delta path", before, after)
    finally:
        ff.close()


@pytest.mark.parametrize("cid", ["fxfy", "double_scale"])
def test_batch_of_eight(mods, cid):
    """k_fuse_surfels<BATCH = true>: eight handles of one configuration in one lock-step step, each with its own crafted frame
    and map (another seed) cut to another length"""
    api, synth, ob = mods
    cam, k, _ = cm.CASES[cid]
    lengths = (63, 64, 65, 200, 256, 257, 1000, None)
    handles, batch = [], None
    try:
        want = []
        for b, n in enumerate(lengths):
            img, dep, pose, ref, surfels, _ = _case(cid, seed=1 + b)
            m = surfels[:n] if n else surfels
            ff, orc = _pair(mods, cid, frame_slots=1, pipeline_depth=1)
            ff.frame_upload(0, img, dep)
            ff.map_upload(m.astype(api.SURFEL_DTYPE))
            handles.append(ff)
            want.append((orc, *orc.fuse_map(ref, img, dep, pose, m)))
        plans = [api.FusionFunctions.pack_replay([0], [_case(cid, seed=1 + b)[3]], _case(cid, seed=1 + b)[2][None]) for b in range(8)]
        batch = api.Batch(handles)
        s, r, p, nf = api.Batch.pack(plans)
        batch.replay_enqueue(s, r, p, nf)
        batch.synchronize()
        for b, (ff, (orc, lo, ko)) in enumerate(zip(handles, want)):
            assert ff.last_new_count() == ko, (cid, b)
            _compare_frame(f"{cid} batched handle {b} ({lengths[b]} records)", ff, orc, ff.map_download(), lo.astype(api.SURFEL_DTYPE))
    finally:
        if batch is not None:
            batch.close()
        for h in handles:
            h.close()


def test_frame_group(mods):
    """the crafted map, then eight frames through replay_enqueue at pipeline_depth 8 (frame groups of four): the crafted
    frame and the scene's next seven; the state after each group equals the oracle's, which fuses frame by frame"""
    api, synth, ob = mods
    cid = "fxfy"
    cam = cm.CASES[cid][0]
    img, dep, pose, ref, surfels, _ = _case(cid)
    scene = synth.Scene(seed=1001, hole_fraction=0.01)
    frames = [(img, dep, pose, ref)]
    for t in range(4, 11):
        i, d, p = synth.render(cam, scene, t)
        frames.append((i, d, cm.tilt(p), ref + (t - 3) // 3))
    ff, orc = _pair(mods, cid, frame_slots=8, pipeline_depth=8)
    try:
        for t, (i, d, _, _) in enumerate(frames):
            ff.frame_upload(t, i, d)
        ff.map_upload(surfels.astype(api.SURFEL_DTYPE))
        slots, refs, poses = api.FusionFunctions.pack_replay(list(range(8)), [f[3] for f in frames], np.stack([f[2] for f in frames]))
        lo = surfels
        for g in (0, 4):
            ff.replay_enqueue(slots[g:g + 4], refs[g:g + 4], poses[g:g + 4])
            ff.synchronize()
            for i, d, p, r in frames[g:g + 4]:
                lo, ko = orc.fuse_map(r, i, d, p, lo)
            assert ff.last_new_count() == ko
            _compare_frame(f"frames {g}..{g + 3}", ff, orc, ff.map_download(), lo.astype(api.SURFEL_DTYPE))
    finally:
        ff.close()


@pytest.mark.parametrize("cid", ["fxfy", "double_focal"])
def test_eigen33_products(mods, cid):
    """DSM_FLAG_EIGEN33_PRODUCTS on crafted input against PortOracle(eigen33=True) (checked on the CPU against the fixtures
    recorded from the reference built with an Eigen >= 3.3 stand-in); the flag moves at least one normal"""
    api, synth, ob = mods
    _dropin_two_frames(mods, cid, eigen33=True)
    img, dep, pose, ref, surfels, _ = _case(cid)
    local = []
    for e33 in (True, False):  # (fuse_initialize_map: no compaction, the records keep their places)
        ff, orc = _pair(mods, cid, eigen33=e33)
        try:
            lg, ng = ff.fuse_initialize_map(ref, img, dep, pose, surfels.astype(api.SURFEL_DTYPE))
            lo, no = orc.fuse_initialize_map(ref, img, dep, pose, surfels)
            assert fields_equal(lg, lo.astype(api.SURFEL_DTYPE)) == [] and fields_equal(ng, no.astype(api.SURFEL_DTYPE)) == [], (cid, e33)
            local.append(lg)
        finally:
            ff.close()
    moved = sum(int((local[0][f].view("u4") != local[1][f].view("u4")).sum()) for f in ("nx", "ny", "nz"))
    assert moved > 0, "the flagged and the unflagged run agree in every normal: the flag was not exercised"


def test_depth_u16(mods):
    """the crafted frame quantised to uint16 = metres * 5000 and converted on the device, the map crafted from that frame,
    against the oracle fed api.depth_from_u16 of it"""
    api, synth, ob = mods
    cid = "double_focal"
    img, dep, pose, ref, surfels, _ = _case(cid, u16_scale=5000.0)
    u16 = np.rint(dep.astype(np.float64) * 5000.0).astype(np.uint16)
    assert np.array_equal(api.depth_from_u16(u16, 5000.0).view("u4"), dep.view("u4"))
    ff, orc = _pair(mods, cid, frame_slots=1)
    try:
        ff.map_upload(surfels.astype(api.SURFEL_DTYPE))
        ff.frame_upload_u16(0, img, u16, 5000.0)
        ff.fuse_frame_resident(0, ref, pose)
        ff.synchronize()
        lo, ko = orc.fuse_map(ref, img, api.depth_from_u16(u16, 5000.0), pose, surfels)
        assert ff.last_new_count() == ko
        after, _ = orc.fuse_initialize_map(ref, img, api.depth_from_u16(u16, 5000.0), pose, surfels)
        oc = cm.outcomes(surfels, after)
        assert int((oc == "fused").sum()) >= 100 and int((oc == "deleted").sum()) >= 8, "the quantised frame left the map little to do"
        _compare_frame("uint16 depth", ff, orc, ff.map_download(), lo.astype(api.SURFEL_DTYPE))
    finally:
        ff.close()
