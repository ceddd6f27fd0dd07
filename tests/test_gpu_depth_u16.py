"""Sensor-native uint16 depth converted to metres on the device (include/dsm.h, the *_u16 entry points).

  1. every u16 value through every u16 form, read back from the slot (dsm_debug_get_frame): equal to api.depth_from_u16 bit
     for bit, for the divide and multiply conventions;
  2. the reference-TU vectors of tum_room / tum_sparse (long_golden.json) through dsm_frame_upload_u16 in the live-callback form;
  3. the batched / streamed forms (dsm_frames_upload_async_u16 double-buffered over a batch of eight, replay.HipEngine with
     depth_u16) against the float forms and the vectors;
  4. 1226x370 with KITTI-style u16 / 256 depth: dsm_replay_enqueue_host_u16 and dsm_frames_upload_async_u16 against the float
     path fed the host-converted frames and against PortOracle;
  5. the node: depth_input_u16 against depth_input of the host-converted frames (state, saved cloud, raw cloud);
  6. argument checks.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import ROOT, fields_equal
from node_state import _canon

pytestmark = pytest.mark.gpu

# (scale, op) pairs of the exhaustive conversion: TUM 5000, KITTI-style 256, millimetres as depth_image_proc multiplies them
CONVERSIONS = [(1.0, "divide"), (256.0, "divide"), (1000.0, "divide"), (5000.0, "divide"), (4096.5, "divide"),
               (0.001, "multiply"), (0.0002, "multiply")]


@pytest.fixture(scope="module")
def mods(oracle_built):
    import torch
    torch.cuda.init()  # torch's HIP runtime first (see __graft_entry__.build)
    from densesurfelmapping_amd import api, synth
    from oracle import bindings
    return api, synth, bindings


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "long_golden.json")))


def map_sha(a, dtype):
    return hashlib.sha256(_canon(np.ascontiguousarray(a, dtype))).hexdigest()


def _all_values(h, w, seed):
    """every uint16 value once (the rest of the frame repeats a shuffled prefix), shuffled"""
    rng = np.random.default_rng(seed)
    v = np.arange(65536, dtype=np.uint16)
    rng.shuffle(v)
    return np.resize(v, h * w).reshape(h, w), rng.integers(0, 256, size=(h, w), dtype=np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_TUM_CACHE = {}


def _tum_frames(synth, case, n):
    """(t, image, u16, pose, ref) of the case's first n frames; the float depth of render() is depth_from_u16(u16, 5000)"""
    cam, scene = getattr(synth, case["camera"]), synth.Scene(**case["scene"])
    out = []
    for t in range(n):
        tl = t % scene.frames_per_period
        key = (case["name"], tl)
        if key not in _TUM_CACHE:
            _TUM_CACHE[key] = synth.render_u16(cam, scene, tl)[:2]
        img, u16 = _TUM_CACHE[key]
        out.append((t, img, u16, scene.pose(t), t // case["keyframe_every"]))
    return cam, scene, out


# ------------------------------------------------------------------ 1. exhaustive conversion
@pytest.mark.parametrize("size", [(256, 256), (250, 263)], ids=["256x256", "250x263_ragged"])
def test_every_u16_value_through_every_form(mods, size):
    """256x256 holds every u16 value once; 250x263 (pitch 256: tight rows differ from pitched, and rows end in a partial vector
    of eight) holds them all too.  Every form must leave the slot's float plane equal to the host conversion, bit for bit."""
    import torch
    api, synth, ob = mods
    w, h = size
    cam = synth.Camera(w, h, 200.0, 200.0, (w - 1) / 2, (h - 1) / 2, far=6.0, near=0.3, rgbd=True)
    u16, img = _all_values(h, w, seed=w)
    assert np.unique(u16).size == 65536
    S = 4
    for scale, op in CONVERSIONS:
        want = api.depth_from_u16(u16, scale, op)
        assert want.dtype == np.float32 and (want[u16 == 0] == 0).all() and not np.signbit(want[u16 == 0]).any()
        tag = f"{w}x{h} {op} {scale}"

        def check(ff, slot, form):
            gi, gd = ff.frame(slot)
            assert np.array_equal(gi, img), f"{tag} {form}: image"
            bad = int((_bits(gd) != _bits(want)).sum())
            assert bad == 0, f"{tag} {form}: {bad} depth values differ, first {np.argwhere(_bits(gd) != _bits(want))[:3].tolist()}"

        for flags in (0, api.DSM_FLAG_UPLOAD_STREAM):
            ff = api.FusionFunctions.from_camera(cam, frame_slots=S, surfel_capacity=1 << 16, flags=flags)
            pitch = ff.frame_pitch()
            # synchronous: tight rows, rows at the slot pitch, rows with some other step (a cv::Mat ROI)
            ff.frame_upload_u16(0, img, u16, scale, op)
            check(ff, 0, f"sync flags={flags} tight")
            buf = np.zeros((h, pitch), np.uint16)
            buf[:, :w] = u16
            ff.frame_upload_u16(1, img, buf[:, :w], scale, op)
            check(ff, 1, f"sync flags={flags} pitched")
            roi = np.zeros((h, w + 3), np.uint16)
            roi[:, 1:w + 1] = u16
            ff.frame_upload_u16(2, img, roi[:, 1:w + 1], scale, op)
            check(ff, 2, f"sync flags={flags} roi")
            ff.close()
        ff = api.FusionFunctions.from_camera(cam, frame_slots=S, surfel_capacity=1 << 16)
        pitch = ff.frame_pitch()
        # device sources: tight, an even step read in place, an odd address (staged)
        dimg = torch.from_numpy(img.copy()).cuda()
        dd = torch.from_numpy(u16.view(np.int16).copy()).cuda()
        ff.frame_upload_device_u16(0, dimg.data_ptr(), w, dd.data_ptr(), 2 * w, scale, op)
        check(ff, 0, "device tight")
        wide = np.zeros((h, w + 5), np.uint16)
        wide[:, :w] = u16
        dw = torch.from_numpy(wide.view(np.int16).copy()).cuda()
        ff.frame_upload_device_u16(1, dimg.data_ptr(), w, dw.data_ptr(), 2 * (w + 5), scale, op)
        check(ff, 1, "device strided")
        odd = np.zeros(h * w * 2 + 1, np.uint8)
        odd[1:] = u16.view(np.uint8).ravel()
        do = torch.from_numpy(odd).cuda()
        ff.frame_upload_device_u16(2, dimg.data_ptr(), w, do.data_ptr() + 1, 2 * w, scale, op)
        check(ff, 2, "device odd address")
        torch.cuda.synchronize()
        # asynchronous: one frame, then batched with pitched rows and with tight rows
        pin = api.PinnedFrames(ff, S, depth_u16=(scale, op))
        tight = api.PinnedFrames(ff, S, tight=True, depth_u16=(scale, op))
        assert pin.depth(0).dtype == np.uint16 and pin.pitch == pitch and tight.pitch == w
        for i in range(S):
            pin.set(i, img, u16)
        tight.set_many(0, [img] * S, [u16] * S)
        ff.frame_upload_async_u16(3, pin.image(0), pin.depth(0), scale, op)
        ff.frame_uploads_wait()
        check(ff, 3, "async single")
        ff.frames_upload_async(0, pin, 0, S)
        ff.frame_uploads_wait()
        for s in range(S):
            check(ff, s, f"async batched pitched, slot {s}")
        ff.frames_upload_async(0, tight, 0, S)
        ff.frame_uploads_wait()
        for s in range(S):
            check(ff, s, f"async batched tight, slot {s}")
        ff.close()
        # frames that come with the enqueue call (frame f -> slot f mod pipeline_depth); the frames are fused too: values far
        # outside a sensor's range may be reported at the next synchronisation, which this test does not make
        ff = api.FusionFunctions.from_camera(cam, frame_slots=4, surfel_capacity=1 << 18, pipeline_depth=4)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        ff.replay_enqueue_host(pin, 0, np.zeros(4, np.int32), np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (4, 1)))
        for s in range(4):
            check(ff, s, f"enqueue_host, slot {s}")
        ff.close()
        pin.close()
        tight.close()
        # the node: the frame waits for its pose at 2 bytes a pixel and goes up through dsm_frame_upload_u16
        from densesurfelmapping_amd import surfel_map
        node = surfel_map.SurfelMap(cam, drift_free_poses=3)
        stamp = (1000, 0)
        node.image_input(stamp, img)
        node.depth_input_u16(stamp, u16, scale, op)
        cov = np.zeros(36)
        cov[0] = 1.0
        eye7 = synth.pose7(np.eye(4))
        node.orb_results_input(stamp, np.zeros(0, np.float32), eye7[None], eye7, cov)
        assert node.frames_fused == 1
        gi = np.zeros((h, w), np.uint8)
        gd = np.zeros((h, w), np.float32)
        lib = api.load_library()
        assert lib.dsm_debug_get_frame(node._lib.dsm_surfel_map_engine(node._h), 0, gi.ctypes.data_as(C.c_void_p), gd.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(gi, img) and np.array_equal(_bits(gd), _bits(want)), f"{tag} node"
        node.close()


# ------------------------------------------------------------------ 2. reference-TU vectors through the u16 upload
@pytest.mark.parametrize("which", [0, 1], ids=["tum_room", "tum_sparse"])
def test_tum_live_callback_form_u16(mods, gold, which):
    """test_tum_live_callback_form's sequence with the frames as the TUM PNGs hold them (uint16, metres x 5000): every frame
    through dsm_frame_upload_u16 into one of two slots in turn, one graph replay, per frame the label image and the surfel
    counts, every checkpoint the whole map -- against the reference TU's vectors."""
    api, synth, ob = mods
    case = gold["tum_sequences"][which]
    cam, scene, frames = _tum_frames(synth, case, case["frames"])
    per = case["per_frame"]
    ff = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=1 << 18)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    for (t, img, u16, pose, ref), want in zip(frames, per):
        ff.frame_upload_u16(t & 1, img, u16, 5000.0, "divide")
        ff.fuse_frame_resident(t & 1, ref, pose)
        ff.synchronize()
        assert (ff.last_new_count(), ff.map_size()) == (want["n_new"], want["n_local"]), f"frame {t}"
        assert hashlib.sha256(ff.labels().tobytes()).hexdigest() == want["labels_sha256"], f"frame {t}: label image"
        if str(t + 1) in case["map_sha256"]:
            assert map_sha(ff.map_download(), api.SURFEL_DTYPE) == case["map_sha256"][str(t + 1)], f"map after frame {t}"
    ff.close()


# ------------------------------------------------------------------ 3. batched and streamed forms
def _batch_streamed(api, cam, frames, B, C, depth_u16):
    """frames through a batch of B handles, chunks of C double-buffered (upload chunk k + 1, then enqueue chunk k); the maps at
    every chunk boundary (of handle 0) and the handles' final maps"""
    hs = [api.FusionFunctions.from_camera(cam, frame_slots=2 * C, surfel_capacity=1 << 18, pipeline_depth=1) for _ in range(B)]
    for h in hs:
        h.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    n = len(frames)
    pin = api.PinnedFrames(hs[0], 2 * C, depth_u16=depth_u16)
    batch = api.Batch(hs)

    def send(k):
        base = (k & 1) * C
        chunk = frames[k * C:(k + 1) * C]
        pin.set_many(base, [f[1] for f in chunk], [f[2] for f in chunk])
        for h in hs:
            h.frames_upload_async(base, pin, base, len(chunk))

    maps = {}
    send(0)
    for k in range(n // C):
        # (chunk k + 1 overwrites the half of the block chunk k - 1 used: that chunk must have been fused)
        if (k + 1) * C < n:
            batch.synchronize()
            send(k + 1)
        chunk = frames[k * C:(k + 1) * C]
        pl = api.FusionFunctions.pack_replay([(k & 1) * C + i for i in range(len(chunk))], [f[4] for f in chunk], [f[3] for f in chunk])
        s_, r_, p_, m = api.Batch.pack([pl] * B)
        batch.replay_enqueue(s_, r_, p_, m)
        batch.synchronize()
        maps[(k + 1) * C] = hs[0].map_download()
    finals = [h.map_download() for h in hs]
    for h in hs:
        h.frame_uploads_wait()
    batch.close()
    for h in hs:
        h.close()
    pin.close()
    return maps, finals


class _U16Source:
    """frames() of a list of (t, image, u16, pose, ref): uint16 depth, or its host conversion"""

    def __init__(self, frames, api=None, scale=None):
        self._f, self._api, self._scale = frames, api, scale

    def frames(self, a, b):
        for t, img, u16, pose, _ in self._f[a:b]:
            yield img, (u16 if self._api is None else self._api.depth_from_u16(u16, self._scale)), pose


@pytest.mark.parametrize("which", [0, 1], ids=["tum_room", "tum_sparse"])
def test_batched_and_streamed_forms_u16(mods, gold, which):
    """60 frames through a batch of eight handles with dsm_frames_upload_async_u16 double-buffered in chunks of ten, and through
    replay.HipEngine(depth_u16=(5000, divide)) (dsm_replay_enqueue_host_u16, frames packed by dsm_host_pack_frames_u16): the maps
    byte-equal to the float forms' and, at the checkpoints, to the reference TU's vectors."""
    api, synth, ob = mods
    from densesurfelmapping_amd import replay
    case = gold["tum_sequences"][which]
    n = 60
    cam, scene, frames = _tum_frames(synth, case, n)
    ffloat = [(t, img, api.depth_from_u16(u16, 5000.0), pose, ref) for t, img, u16, pose, ref in frames]
    maps16, fin16 = _batch_streamed(api, cam, frames, 8, 10, (5000.0, "divide"))
    maps32, fin32 = _batch_streamed(api, cam, ffloat, 8, 10, None)
    for t, m in maps16.items():
        assert _canon(m) == _canon(maps32[t]), f"batched u16 vs float after {t} frames"
        if str(t) in case["map_sha256"]:
            assert map_sha(m, api.SURFEL_DTYPE) == case["map_sha256"][str(t)], f"batched u16 after {t} frames"
    for a, b in zip(fin16, fin32):
        assert _canon(a) == _canon(b)
    assert any(str(t) in case["map_sha256"] for t in maps16)
    # one streamed sequence
    got = {}
    for u in ((5000.0, "divide"), None):
        eng = replay.HipEngine(cam, capacity=1 << 18, chunk=16, depth_u16=u)
        src = _U16Source(frames) if u else _U16Source(frames, api, 5000.0)
        for a, b in ((0, 40), (40, n)):
            eng.replay(src, a, b, keyframe_every=case["keyframe_every"], origin=0)
            m = eng.cloud()
            got[(u is None, b)] = m
            if str(b) in case["map_sha256"]:
                assert map_sha(m, api.SURFEL_DTYPE) == case["map_sha256"][str(b)], f"HipEngine depth_u16={u} after {b} frames"
        eng.close()
    for b in (40, n):
        assert _canon(got[(False, b)]) == _canon(got[(True, b)]), f"HipEngine u16 vs float after {b} frames"
        assert _canon(got[(False, b)]) == _canon(maps16[b]), f"HipEngine vs batch after {b} frames"


# ------------------------------------------------------------------ 4. 1226x370, KITTI-style u16 / 256
def test_kitti_u16_256(mods):
    """a `drive` sequence quantised to uint16 / 256 (KITTI-style depth PNGs): dsm_replay_enqueue_host_u16 (frame groups) and
    dsm_frames_upload_async_u16 + dsm_replay_enqueue against the float path fed the host-converted frames, and against PortOracle"""
    api, synth, ob = mods
    cam, scene = synth.KITTI_1226, synth.Scene()
    n = 16
    frames = []
    for t, img, dep, pose, ref in synth.sequence(cam, scene, n):
        u16 = np.clip(np.round(dep.astype(np.float64) * 256.0), 0, 65535).astype(np.uint16)
        frames.append((t, img, u16, pose, ref))
    conv = [api.depth_from_u16(f[2], 256.0) for f in frames]
    assert all((c[f[2] > 0] > 0).all() for c, f in zip(conv, frames)) and np.mean([np.unique(f[2]).size for f in frames]) > 1000
    poses = np.stack([api.pose_to_colmajor(f[3]) for f in frames])
    refs = np.array([f[4] for f in frames], np.int32)
    # the float path, frame by frame, and the oracle
    ff = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=1 << 20)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    orc = ob.PortOracle(cam)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    for (t, img, u16, pose, ref), dep in zip(frames, conv):
        ff.frame_upload(t & 1, img, dep)
        ff.fuse_frame_resident(t & 1, ref, pose)
        lo, ko = orc.fuse_map(ref, img, dep, pose, lo)
        assert ff.last_new_count() == ko, f"frame {t}"
    want = ff.map_download()
    assert not fields_equal(want, lo.astype(api.SURFEL_DTYPE)), "float path vs PortOracle"
    want_labels = ff.labels()
    assert np.array_equal(want_labels, orc.labels())
    ff.close()
    # frames coming with the enqueue call, u16 (pipeline depth 8: groups of four, each converted behind its copy)
    ff = api.FusionFunctions.from_camera(cam, frame_slots=8, surfel_capacity=1 << 20, pipeline_depth=8)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    pin = api.PinnedFrames(ff, n, depth_u16=(256.0, "divide"))
    pin.set_many(0, [f[1] for f in frames], [f[2] for f in frames])
    ff.replay_enqueue_host(pin, 0, refs[:8], poses[:8])
    ff.replay_enqueue_host(pin, 8, refs[8:], poses[8:])
    got = ff.map_download()
    assert _canon(got) == _canon(want), "dsm_replay_enqueue_host_u16"
    assert np.array_equal(ff.labels(), want_labels)
    ff.close()
    # asynchronous uploads in two chunks of eight (tight rows), then one enqueue each
    ff = api.FusionFunctions.from_camera(cam, frame_slots=16, surfel_capacity=1 << 20)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    tight = api.PinnedFrames(ff, n, tight=True, depth_u16=(256.0, "divide"))
    tight.set_many(0, [f[1] for f in frames], [f[2] for f in frames])
    ff.frames_upload_async(0, tight, 0, 8)
    ff.frames_upload_async(8, tight, 8, 8)
    for c0 in (0, 8):
        s_, r_, p_ = ff.pack_replay(list(range(c0, c0 + 8)), refs[c0:c0 + 8], [f[3] for f in frames[c0:c0 + 8]])
        ff.replay_enqueue(s_, r_, p_)
    got = ff.map_download()
    assert _canon(got) == _canon(want), "dsm_frames_upload_async_u16"
    ff.frame_uploads_wait()
    ff.close()
    pin.close()
    tight.close()


# ------------------------------------------------------------------ 5. the node
def test_node_depth_input_u16(mods, tmp_path):
    """a TUM-style message log (RGB-D constant set, a closed loop, keyframes every four frames) fed once with depth_input_u16 and
    once with depth_input of the host-converted frames: the final node state, the saved cloud and the raw cloud byte-equal"""
    api, synth, ob = mods
    import node_state
    from densesurfelmapping_amd import surfel_map
    cam = synth.NODE_CAM_RGBD
    scene = synth.Scene(seed=5, tum=True, frames_per_period=32, intensity_noise=8.0, checker=25.0, n_boxes=6)
    rendered = {tl: synth.render_u16(cam, scene, tl)[:2] for tl in range(32)}
    out = {}
    for use_u16 in (True, False):
        frames = rendered if use_u16 else {tl: (img, api.depth_from_u16(u, 5000.0)) for tl, (img, u) in rendered.items()}
        node = surfel_map.SurfelMap(cam, drift_free_poses=3)
        for ev in synth.node_messages(cam, scene, 44, lap=32, keyframe_every=4, drift_rate=0.1, frames=frames):
            if ev[0] == "depth" and use_u16:
                assert ev[2].dtype == np.uint16
                node.depth_input_u16(ev[1], ev[2], 5000.0, "divide")
            else:
                node.feed(ev)
        assert node.frames_fused == 44
        path = str(tmp_path / f"cloud_{int(use_u16)}.pcd")
        node.save_cloud(path)
        out[use_u16] = (node_state.digest(node_state.snapshot(node)), node_state.file_digest(path)["sha256"], _canon(node.cloud("raw")),
                        len(node.local_surfels()))
        node.close()
    assert out[True][3] > 1000, "the log fused next to nothing"
    assert out[True][0] == out[False][0], "node state"
    assert out[True][1] == out[False][1], "saved cloud"
    assert out[True][2] == out[False][2], "raw cloud"


# ------------------------------------------------------------------ 6. arguments
def test_u16_arguments_refused(mods):
    """bad scale / op / step / pointer / slot: DSM_E_INVALID before any device work; 16UC1 through depth_input is still refused"""
    api, synth, ob = mods
    from densesurfelmapping_amd import surfel_map
    lib = api.load_library()
    cam = synth.TINY
    w, h = cam.width, cam.height
    ff = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=1 << 16, pipeline_depth=1)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    img = np.zeros((h, w), np.uint8)
    u16 = np.full((h, w), 1000, np.uint16)
    pin = api.PinnedFrames(ff, 2, depth_u16=(1000.0, "divide"))
    H = ff._h
    vp = C.c_void_p
    P = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (2, 1))
    refs = np.zeros(2, np.int32)
    pi, pd = pin.image(0), pin.depth(0)
    calls = {
        "sync": lambda s, op, st=2 * w, slot=0, d=P(u16): lib.dsm_frame_upload_u16(H, slot, P(img), w, d, st, s, op),
        "device": lambda s, op, st=2 * w, slot=0, d=P(u16): lib.dsm_frame_upload_device_u16(H, slot, P(img), w, d, st, s, op),
        "async": lambda s, op, st=2 * pin.pitch, slot=0, d=P(pd): lib.dsm_frame_upload_async_u16(H, slot, P(pi), pi.strides[0], d, st, s, op),
        "async_n": lambda s, op, st=2 * pin.pitch, slot=0, d=P(pd): lib.dsm_frames_upload_async_u16(
            H, slot, 2, P(pi), pi.strides[0], pin.pitch * h, d, st, pin.pitch * h * 2, s, op),
        "enqueue_host": lambda s, op, st=2 * pin.pitch, slot=0, d=P(pd): lib.dsm_replay_enqueue_host_u16(
            H, 2, P(pi), pi.strides[0], pin.pitch * h, d, st, pin.pitch * h * 2, P(refs), P(eye), None, s, op),
    }
    for name, call in calls.items():
        for s, op in ((0.0, 0), (-1.0, 0), (float("nan"), 0), (float("inf"), 1), (-0.0, 1), (1000.0, 2), (1000.0, -1)):
            assert call(s, op) == api.DSM_E_INVALID, (name, s, op)
        assert call(1000.0, 0, st=2 * w - 1) == api.DSM_E_INVALID, (name, "step")
        assert call(1000.0, 0, d=None) == api.DSM_E_INVALID, (name, "null depth")
        if name != "enqueue_host":
            assert call(1000.0, 0, slot=-1) == api.DSM_E_INVALID, (name, "slot -1")
            assert call(1000.0, 0, slot=2) == api.DSM_E_INVALID, (name, "slot 2")
    assert lib.dsm_debug_get_frame(H, 2, None, None) == api.DSM_E_INVALID
    assert lib.dsm_debug_get_frame(H, -1, None, None) == api.DSM_E_INVALID
    # nothing went to the device: the handle is clean and still works
    ff.frame_upload_u16(0, img, u16, 1000.0, "divide")
    assert np.array_equal(ff.frame(0)[1], api.depth_from_u16(u16, 1000.0))
    assert np.array_equal(ff.frame(0)[1], np.ones((h, w), np.float32))
    with pytest.raises(TypeError):
        ff.frame_upload_u16(0, img, u16.astype(np.float32), 1000.0)
    with pytest.raises(KeyError):
        ff.frame_upload_u16(0, img, u16, 1000.0, "log")
    ff.close()
    pin.close()
    assert lib.dsm_host_pack_frames_u16(1, w, h, None, None, None, None, None, w, w * h, None, 2 * w, 2 * w * h) == api.DSM_E_INVALID
    node = surfel_map.SurfelMap(cam, drift_free_poses=3)
    with pytest.raises(api.DsmError) as e:
        node.depth_input((1000, 0), u16.view(np.uint16), encoding="16UC1")
    assert e.value.code == api.DSM_E_INVALID
    for s, op, enc in ((0.0, "divide", "16UC1"), (float("nan"), "divide", "16UC1"), (1.0, 7, "16UC1"), (1.0, "divide", "32FC1")):
        with pytest.raises(api.DsmError) as e:
            node.depth_input_u16((1000, 0), u16, s, op, encoding=enc)
        assert e.value.code == api.DSM_E_INVALID, (s, op, enc)
    node.close()
