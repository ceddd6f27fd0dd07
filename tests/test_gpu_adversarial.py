"""Adversarial parity of the batched forms: the lane-per-seed kernels (launches over eight handles or more, and the frame
groups of one sequence), the queues behind them and the drop-in delta download's shrinking calls.

test_edge_inputs feeds NaN, +-inf, negative depths, noise and exact cost ties to ONE handle, which runs the wave-per-seed
kernels.  Here the same frames and two longer hostile sequences go through the forms the headline runs:

  * k_init_seeds_lanes, k_assign<..., 4>, k_update_seeds + k_update_seeds_rest, k_pixel_normals + k_seed_stats;
  * k_update_seeds_rest's two queues: seeds that need more Huber passes (kQueueRest, large on pure noise) and seeds whose
    depth list outgrew its LDS row (kQueueWave, filled by few grey levels over stereo depth);
  * both tiers of k_seed_fit in a batched launch, with the short tier's limit lowered so the full-length tier takes
    ordinary groups.

Every handle is compared with PortOracle (the C restatement) after EVERY frame -- label image, seed table, surfel array and
the new-surfel count, every byte equal, NaN == NaN -- and every test asserts through dsm_debug_tier_counts /
dsm_debug_dropin_stats that the path it is about actually ran.
"""
import concurrent.futures
import hashlib

import numpy as np
import pytest

from conftest import fields_equal
from test_gpu_parity import _compare_frame, edge_cases

pytestmark = pytest.mark.gpu

B = 8  # handles per batch: kLaneBatch, the smallest batch that takes the lane-per-seed forms


@pytest.fixture(scope="module")
def mods(oracle_built):
    import torch
    torch.cuda.init()
    from densesurfelmapping_amd import api, synth
    from oracle import bindings
    return api, synth, bindings


def _digest(a):
    """Hash of an array's values field by field (no padding bytes), every float NaN made the same NaN: equal digests = every
    byte equal, NaN == NaN (the bar of fields_equal)."""
    h = hashlib.sha1()
    for f in a.dtype.names or (None,):
        x = np.array(a[f] if f else a)
        if x.dtype.kind == "f":
            x[np.isnan(x)] = np.nan
        h.update(x.tobytes())
    return h.hexdigest()


def _gpu_record(ff):
    return ff.last_new_count(), ff.map_size(), _digest(ff.labels()), _digest(ff.seeds()), _digest(ff.map_download())


def _oracle_replay(ob, cam, frames):
    """frames [(image, depth, pose, ref)] through one PortOracle: a record per frame (as _gpu_record) and the last state."""
    orc = ob.PortOracle(cam)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    recs = []
    for img, dep, pose, ref in frames:
        lo, k = orc.fuse_map(ref, img, dep, pose, lo)
        recs.append((k, len(lo), _digest(orc.labels()), _digest(orc.seeds()), _digest(lo)))
    return recs, orc, lo


def _oracle_replays(ob, cam, runs):
    # one oracle per handle, on threads (the C oracle keeps no global state, ctypes lets go of the GIL)
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(runs)) as ex:
        return list(ex.map(lambda fr: _oracle_replay(ob, cam, fr), runs))


_RECORD = ("new surfel count", "map size", "label image", "seed table", "surfel array")


def _check_record(tag, got, want):
    bad = [name for name, g, w in zip(_RECORD, got, want) if g != w]
    assert not bad, f"{tag}: {bad} differ from the oracle (counts {got[:2]} vs {want[:2]})"


def _check_final(tag, api, ff, orc, lo):
    _compare_frame(tag, ff, orc, ff.map_download(), lo.astype(api.SURFEL_DTYPE))


def _batched_lockstep(api, cam, runs, want, fit_small_cap=None, tag=""):
    """Eight handles, handle b fed runs[b] = [(image, depth, pose, ref)], advanced as ONE batch a frame at a time, every handle
    checked against its oracle record after every frame; returns the tier counts [frame][handle]."""
    n = len(runs[0])
    handles, batch = [], None
    try:
        for fr in runs:
            ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=1 << 20, pipeline_depth=1)
            if fit_small_cap is not None:
                ff.debug_set_fit_small_cap(fit_small_cap)
            for t, (img, dep, _, _) in enumerate(fr):
                ff.frame_upload(t, img, dep)
            ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
            handles.append(ff)
        plans = [api.FusionFunctions.pack_replay(list(range(n)), [f[3] for f in fr], np.stack([f[2] for f in fr])) for fr in runs]
        batch = api.Batch(handles)
        tiers = []
        for t in range(n):
            s, r, p, m = api.Batch.pack([(pl[0][t:t + 1], pl[1][t:t + 1], pl[2][t:t + 1]) for pl in plans])
            batch.replay_enqueue(s, r, p, m)
            batch.synchronize()
            tiers.append([h.debug_tier_counts() for h in handles])
            for b, h in enumerate(handles):
                _check_record(f"{tag} handle {b} frame {t}", _gpu_record(h), want[b][0][t])
        for b, h in enumerate(handles):
            _check_final(f"{tag} handle {b} after {n} frames", api, h, want[b][1], want[b][2])
        return tiers
    finally:
        if batch is not None:
            batch.close()
        for h in handles:
            h.close()


# ---------------------------------------------------------------------------------------------------------------------
# (1, 2, 5) test_edge_inputs' hostile frames, one case per handle, through batches of eight

@pytest.fixture(scope="module")
def edge_oracle(mods):
    """camera -> (case names, {case: frames}, {case: oracle replay}); a case = the frame twice (initialisation, then fusion into
    the map it made), identity pose, as test_edge_inputs."""
    api, synth, ob = mods
    cache = {}

    def get(camera):
        if camera not in cache:
            cam = getattr(synth, camera)
            pose = np.eye(4, dtype=np.float32)
            frames = {name: [(img, dep, pose, 0), (img, dep, pose, 1)] for name, (img, dep) in edge_cases(cam).items()}
            names = list(frames)
            cache[camera] = (names, frames, dict(zip(names, _oracle_replays(ob, cam, [frames[c] for c in names]))))
        return cache[camera]
    return get


@pytest.mark.parametrize("camera,fit_small_cap", [("KITTI_1226", None), ("KITTI_1226", 0), ("KITTI_1226", 40),
                                                  ("TINY_RAGGED", None), ("KITTI_1241", None)])
def test_lane_form_edge_inputs(mods, edge_oracle, camera, fit_small_cap):
    """The eleven cases of test_edge_inputs over two batches of eight handles (the second batch: the last three cases and the
    first five again), a different case in every handle of a batch.  TINY_RAGGED (166x103) has (size mod 8) > 4: its last
    columns and rows have no candidate superpixel and are labelled -1 on both sides; KITTI_1241 is ragged by
    one column.  fit_small_cap 0 / 40 sends every / most groups of four seeds through k_seed_fit's full-length tier."""
    api, synth, ob = mods
    cam = getattr(synth, camera)
    names, frames, want = edge_oracle(camera)
    assert len(names) == 11
    for k, sel in enumerate((names[:B], names[B:] + names[:2 * B - len(names)])):
        tiers = _batched_lockstep(api, cam, [frames[c] for c in sel], [want[c] for c in sel], fit_small_cap,
                                  tag=f"{camera} cap {fit_small_cap} batch {k}")
        flat = [tc for per_frame in tiers for tc in per_frame]
        # the lane forms ran: only k_update_seeds queues seeds for more Huber passes (all zero after a wave-form frame)
        assert any(any(tc["huber_rest_by_sweep"]) for tc in flat), (k, flat)
        if fit_small_cap is not None:
            assert max(tc["fit_long_groups"] for tc in flat) > 0, (k, flat)
        print(camera, fit_small_cap, "batch", k, "huber rest max", max(max(tc["huber_rest_by_sweep"]) for tc in flat),
              "long lists max", max(max(tc["long_list_by_sweep"]) for tc in flat), "fit long groups max", max(tc["fit_long_groups"] for tc in flat))


# ---------------------------------------------------------------------------------------------------------------------
# (3, 4) longer hostile sequences at 1226x370: few grey levels over stereo depth, pure noise

SEQ_FRAMES = {"few_greys": 22, "noise": 30}  # (22 and 30 are not multiples of the frame groups' 4 and 8: ragged ends)


def _noise_frames(synth, cam, n):
    """noise in intensity and depth (0.4-8 m, 15 % holes), the camera creeping forward"""
    scene = synth.Scene(seed=11, step=0.05)
    out = []
    for t in range(n):
        rng = np.random.default_rng(5000 + t)
        img = rng.integers(0, 256, (cam.height, cam.width)).astype(np.uint8)
        dep = np.where(rng.random((cam.height, cam.width)) < 0.15, 0.0, rng.uniform(0.4, 8.0, (cam.height, cam.width))).astype(np.float32)
        out.append((img, dep, scene.pose(t)))
    return out


def _few_grey_frames(synth, cam, n):
    """two grey levels and saturated highlights over stereo depth (disparity-quantised, +inf where it is 0): large superpixels
    of exact cost ties, hundreds per frame with more depths than an LDS row of k_update_seeds holds"""
    scene = synth.Scene(seed=7, stereo=True, intensity_levels=2, saturate_above=120)
    return [synth.render(cam, scene, t) for t in range(n)]


@pytest.fixture(scope="module")
def seq_oracle(mods):
    """sequence -> (runs, oracle replays): handle b of a batch takes frames b .. b + n - 1 (its own keyframes from its first
    frame), so the eight handles see different frames and maps; run 0 is also the frame-group tests' sequence."""
    api, synth, ob = mods
    cam = synth.KITTI_1226
    cache = {}

    def get(seq):
        if seq not in cache:
            n = SEQ_FRAMES[seq]
            fr = (_noise_frames if seq == "noise" else _few_grey_frames)(synth, cam, n + B - 1)
            runs = [[(img, dep, pose, t // 5) for t, (img, dep, pose) in enumerate(fr[b:b + n])] for b in range(B)]
            cache[seq] = (runs, _oracle_replays(ob, cam, runs))
        return cache[seq]
    return get


@pytest.mark.parametrize("seq", ["few_greys", "noise"])
def test_lane_form_hostile_sequences(mods, seq_oracle, seq):
    """A batch of eight handles through 22 few-grey / 30 noise frames.  Few grey levels fill kQueueWave (lists longer than the
    127-entry LDS row, refined by a wave each in k_update_seeds_rest); noise fills kQueueRest (seeds that need a second and
    later Huber pass).  Every handle equals its oracle after every frame."""
    api, synth, ob = mods
    runs, want = seq_oracle(seq)
    tiers = _batched_lockstep(api, synth.KITTI_1226, runs, want, tag=seq)
    flat = [tc for per_frame in tiers for tc in per_frame]
    rest = max(max(tc["huber_rest_by_sweep"]) for tc in flat)
    long_lists = sum(sum(tc["long_list_by_sweep"]) for tc in flat)
    print(seq, "huber rest max", rest, "long lists in all", long_lists, "fit long groups max", max(tc["fit_long_groups"] for tc in flat))
    assert rest > 0, flat
    if seq == "noise":  # (most seeds: noise in depth leaves nearly every list with a Huber step above 0.01 after the first pass)
        cam = synth.KITTI_1226
        assert rest > (cam.width // 8) * (cam.height // 8) // 2, flat  # (one superpixel per 8x8 cell)
    if seq == "few_greys":
        assert long_lists > 0, "no depth list outgrew its LDS row: kQueueWave stayed empty"


@pytest.mark.parametrize("depth", [8, 24], ids=["G4", "G8"])
@pytest.mark.parametrize("seq", ["few_greys", "noise"])
def test_frame_groups_hostile_sequences(mods, seq_oracle, seq, depth):
    """One sequence through one handle with pipeline_depth 8 (frame groups of G = 4) and 24 (G = 8): the superpixel stages of G
    consecutive frames as one batched launch in the lane-per-seed forms (lanes_from = 4), then the ragged end frame by frame.
    The last group's frame and the final state equal the oracle's."""
    api, synth, ob = mods
    cam = synth.KITTI_1226
    runs, want = seq_oracle(seq)
    fr, (recs, orc, lo) = runs[0], want[0]
    n, G = len(fr), {8: 4, 24: 8}[depth]
    grouped = n - n % G
    assert 0 < grouped < n
    ff = api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=1 << 20, pipeline_depth=depth)
    try:
        for t, (img, dep, _, _) in enumerate(fr):
            ff.frame_upload(t, img, dep)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        slots, refs, poses = api.FusionFunctions.pack_replay(list(range(n)), [f[3] for f in fr], np.stack([f[2] for f in fr]))
        ff.replay_enqueue(slots[:grouped], refs[:grouped], poses[:grouped])
        tc = ff.debug_tier_counts()  # (the latest frame's: the last of a group)
        print(seq, depth, "last group:", tc)
        assert any(tc["huber_rest_by_sweep"]), tc
        if seq == "few_greys":
            assert any(tc["long_list_by_sweep"]), tc
        _check_record(f"{seq} depth {depth} frame {grouped - 1}", _gpu_record(ff), recs[grouped - 1])
        ff.replay_enqueue(slots[grouped:], refs[grouped:], poses[grouped:])
        ff.synchronize()
        _check_record(f"{seq} depth {depth} frame {n - 1}", _gpu_record(ff), recs[n - 1])
        _check_final(f"{seq} depth {depth} after {n} frames", api, ff, orc, lo)
    finally:
        ff.close()


# ---------------------------------------------------------------------------------------------------------------------
# (6) the drop-in delta download on a shrinking call

def _parked(api, n, seed):
    """live surfels far behind the camera: never in view, never pruned (update_times >= 5), never touched by a frame"""
    rng = np.random.default_rng(seed)
    a = np.zeros(n, api.SURFEL_DTYPE)
    a["px"] = rng.uniform(-20.0, 20.0, n)
    a["py"] = rng.uniform(-5.0, 5.0, n)
    a["pz"] = -50.0 - rng.uniform(0.0, 10.0, n)
    a["nz"], a["size"], a["color"], a["weight"], a["update_times"] = 1.0, 0.1, 100.0, 1.0, 9
    return a


@pytest.mark.parametrize("aligned", [False, True], ids=["ragged_end", "end_multiple_of_64"])
def test_dropin_delta_download_shrinking_call(mods, aligned):
    """A call that deletes far more surfels than it spawns and still takes the delta path: the map holds parked surfels, then a
    wall's, then parked ones again (appended by the caller); the next frame sees +inf (an unmatched disparity) where the lower
    two thirds of the wall were, which deletes their surfels (FF.cpp:236-240) and spawns none, so the compaction fills the
    holes from the end of the array (SM.cpp:1096-1109, the new-count < holes branch).  The few groups that changes must all
    come back.  Once with the shrunk map ending inside a 64-record group, once on a group boundary."""
    api, synth, ob = mods
    cam = synth.KITTI_1226
    H, W = cam.height, cam.width
    rng = np.random.default_rng(5)
    img = (np.add.outer(np.arange(H) // 8, np.arange(W) // 8) * 37 % 200 + rng.integers(0, 20, (H, W))).astype(np.uint8)
    wall = np.full((H, W), 4.0, np.float32)
    gone = wall.copy()
    gone[H // 3:] = np.inf
    pose = np.eye(4, dtype=np.float32)
    head = _parked(api, 64 * 1000 + 17, 1)

    def oracle(tail_n):
        orc = ob.PortOracle(cam)
        lo, _ = orc.fuse_map(0, img, wall, pose, head.astype(ob.SURFEL_DTYPE))
        lo = np.concatenate([lo, _parked(api, tail_n, 2).astype(ob.SURFEL_DTYPE)])
        out = [lo]
        for ref, dep in ((1, gone), (2, wall)):
            lo, k = orc.fuse_map(ref, img, dep, pose, lo)
            out.append(lo)
        return out
    tail_n = 64 * 800
    if aligned:
        tail_n -= len(oracle(tail_n)[1]) % 64
    want = oracle(tail_n)
    assert len(want[1]) < len(want[0]) and (len(want[1]) % 64 == 0) == aligned
    ff = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=1 << 18)
    try:
        buf = np.zeros(1 << 18, api.SURFEL_DTYPE)
        buf[:len(head)] = head
        n, _ = ff.fuse_map_inplace(0, img, wall, pose, buf, len(head))
        buf[n:n + tail_n] = _parked(api, tail_n, 2)
        n += tail_n
        assert fields_equal(buf[:n], want[0].astype(api.SURFEL_DTYPE)) == []
        for i, (ref, dep) in enumerate(((1, gone), (2, wall))):
            before = ff.debug_dropin_stats()
            m, _ = ff.fuse_map_inplace(ref, img, dep, pose, buf, n)
            after = ff.debug_dropin_stats()
            assert m == len(want[i + 1]) and fields_equal(buf[:m], want[i + 1].astype(api.SURFEL_DTYPE)) == [], f"call {ref}"
            if i == 0:
                assert m < n, (n, m)
                assert after["delta_calls"] == before["delta_calls"] + 1, ("the shrinking call took the full download", before, after)
                print("shrinking call:", n, "->", m, "surfels,", after["last_groups"], "groups back of", (m + 63) // 64)
            n = m
    finally:
        ff.close()
