"""Colour camera images converted to grey on the device (include/dsm.h, dsm_frame_format and the *_fmt entry points).

  1. every channel value through every form and layout, read back from the slot with its pad columns (dsm_debug_frame_planes):
     equal to api.gray_from_color byte for byte, pad bytes untouched;
  2. short sequences through the live, batched, frame-group and enqueue-with-frames forms: labels, seed table and map equal to
     the same form fed the mono8 frames of gray_from_color, and (one form) to PortOracle on those grey frames;
  3. colour + uint16 depth in one call against mono8 + float depth of the host-converted frame;
  4. the node: image_input_color with depth_input and depth_input_u16 against a node fed the grey frames;
  5. argument checks.
"""
import ctypes as C

import numpy as np
import pytest

import color_cases as cc
from conftest import fields_equal
from node_state import _canon

pytestmark = pytest.mark.gpu

# 256x256: no pad columns; 250x263: ragged (pitch 256, rows end in a partial group of four, w * 3 is no multiple of 4 either);
# 25x24: the narrowest size dsm_create takes (3 cells of 8) whose width is no multiple of the kernel's group of four pixels
SIZES = [(256, 256), (250, 263), (25, 24)]
S = 4  # frame slots = frames of a case


@pytest.fixture(scope="module")
def mods(oracle_built):
    import torch
    torch.cuda.init()  # torch's HIP runtime first (see __graft_entry__.build)
    from densesurfelmapping_amd import api, synth
    from oracle import bindings
    return api, synth, bindings


class _Pinned:
    """page-locked bytes (dsm_host_alloc) as a numpy array"""

    def __init__(self, api, n):
        self._lib = api.load_library()
        self._p = C.c_void_p()
        assert self._lib.dsm_host_alloc(C.byref(self._p), n) == 0
        self.a = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_uint8)), shape=(n,))
        self.a[:] = 0x5A

    def close(self):
        self.a = None
        self._lib.dsm_host_free(self._p)


_EXH = {}


def _exhaustive(w, h):
    if (w, h) not in _EXH:
        _EXH[(w, h)] = cc.exhaustive_rgb(h * S, w, seed=w).reshape(S, h, w, 3)
    return _EXH[(w, h)]


# ------------------------------------------------------------------ 1. exhaustive conversion
@pytest.mark.parametrize("enc", cc.ENCODINGS)
@pytest.mark.parametrize("size", SIZES, ids=["256x256", "250x263_ragged", "25x24_narrow"])
def test_every_value_every_form_every_layout(mods, size, enc):
    import torch
    api, synth, ob = mods
    lib = api.load_library()
    w, h = size
    ch = cc.CHANNELS[enc]
    cam = synth.Camera(w, h, 200.0, 200.0, (w - 1) / 2, (h - 1) / 2, far=6.0, near=0.3, rgbd=True)
    rgb = _exhaustive(w, h)
    rng = np.random.default_rng(7)
    col = [cc.to_encoding(rgb[i], enc, rng.integers(0, 256, (h, w), dtype=np.uint8)) for i in range(S)]
    dep = np.zeros((h, w), np.float32)  # (invalid everywhere: the frames that are fused as well fuse nothing)
    ff = api.FusionFunctions.from_camera(cam, frame_slots=S, surfel_capacity=1 << 16)
    ffu = api.FusionFunctions.from_camera(cam, frame_slots=S, surfel_capacity=1 << 16, flags=api.DSM_FLAG_UPLOAD_STREAM)
    ffq = api.FusionFunctions.from_camera(cam, frame_slots=4, surfel_capacity=1 << 16, pipeline_depth=4)
    ffq.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    pitch = ff.frame_pitch()
    steps = [pitch * ch, w * ch, w * ch + 1]
    pattern = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    pin = _Pinned(api, S * h * (pitch * ch + 1) + 64)
    pdep = _Pinned(api, S * h * pitch * 4)
    pdep.a[:] = 0
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (S, 1))
    refs = np.zeros(S, np.int32)
    vp = C.c_void_p

    def prefill(f, slots):
        for s in slots:
            f.frame_planes(s, image=pattern)

    def check(f, slot, want, form):
        got = f.frame_planes(slot)[0]
        bad = int((got[:, :w] != want).sum())
        assert bad == 0, f"{form}: {bad} grey bytes differ, first {np.argwhere(got[:, :w] != want)[:3].tolist()}"
        assert np.array_equal(got[:, w:], pattern[:, w:]), f"{form}: pad bytes were written"

    def host_layout(step):
        """the S frames in page-locked memory, rows `step` bytes apart and frames step * h apart; [frame] -> address"""
        v = np.lib.stride_tricks.as_strided(pin.a, shape=(S, h, w * ch), strides=(step * h, step, 1))
        pin.a[:] = 0x5A
        for i in range(S):
            v[i] = col[i].reshape(h, w * ch)
        return [pin.a.ctypes.data + i * step * h for i in range(S)]

    for name, weights in cc.WEIGHT_SETS.items():
        want = [api.gray_from_color(c, enc, weights) for c in col]
        fmt = api.frame_format(enc, weights)
        tag = f"{w}x{h} {enc} {name}"
        # synchronous: rows at the slot pitch, tight rows, an odd step; on the map stream and on an upload stream of the handle's own
        for f, fl in ((ff, "sync"), (ffu, "sync upload-stream")):
            prefill(f, range(3))
            for s, step in enumerate(steps):
                f.frame_upload_fmt(s, cc.strided(col[s], step)[0], dep, fmt)
                check(f, s, want[s], f"{tag} {fl} step {step}")
        # device memory, read in place: tight rows, rows at the pitch, tight rows at an odd base address
        prefill(ff, range(3))
        dd = torch.from_numpy(dep).cuda()
        keep = []
        for s, (step, off) in enumerate(((w * ch, 0), (pitch * ch, 0), (w * ch, 1))):
            raw = np.zeros(h * step + 16, np.uint8)
            np.lib.stride_tricks.as_strided(raw[off:], shape=(h, w * ch), strides=(step, 1))[:] = col[s].reshape(h, w * ch)
            d = torch.from_numpy(raw).cuda()
            keep.append(d)
            ff.frame_upload_device_fmt(s, d.data_ptr() + off, step, dd.data_ptr(), 4 * w, fmt)
            check(ff, s, want[s], f"{tag} device step {step} offset {off}")
        torch.cuda.synchronize()
        # asynchronous, one frame and S frames; frames that come with the enqueue call (frame f -> slot f mod 4)
        for step in steps:
            addr = host_layout(step)
            prefill(ff, range(S))
            assert lib.dsm_frame_upload_async_fmt(ff._h, 3, vp(addr[1]), step, vp(pdep.a.ctypes.data), pitch * 4, C.byref(fmt)) == 0
            check(ff, 3, want[1], f"{tag} async single step {step}")
            ff.frame_planes(3, image=pattern)
            assert lib.dsm_frames_upload_async_fmt(ff._h, 0, S, vp(addr[0]), step, step * h, vp(pdep.a.ctypes.data), pitch * 4, pitch * h * 4, C.byref(fmt)) == 0
            for s in range(S):
                check(ff, s, want[s], f"{tag} async x{S} step {step} slot {s}")
            ff.frame_uploads_wait()
            prefill(ffq, range(S))
            assert lib.dsm_replay_enqueue_host_fmt(ffq._h, S, vp(addr[0]), step, step * h, vp(pdep.a.ctypes.data), pitch * 4, pitch * h * 4,
                                                   refs.ctypes.data_as(vp), eye.ctypes.data_as(vp), None, C.byref(fmt)) == 0
            for s in range(S):
                check(ffq, s, want[s], f"{tag} enqueue_host step {step} slot {s}")
            ffq.replay_wait()
    # the Python mirror of the page-locked layouts (PinnedFrames(image_format=...)), pitched and tight
    weights = cc.WEIGHT_SETS["opencv15"]
    want = [api.gray_from_color(c, enc, weights) for c in col]
    for tight in (False, True):
        blk = api.PinnedFrames(ff, S, tight=tight, image_format=enc, gray_weights=weights)
        assert blk.image(0).shape == (h, w, ch) and blk.image(0).strides[0] == (w if tight else pitch) * ch
        blk.set_many(0, col, [dep] * S)
        prefill(ff, range(S))
        ff.frames_upload_async(0, blk, 0, S)
        for s in range(S):
            check(ff, s, want[s], f"PinnedFrames tight={tight} slot {s}")
        ff.frame_uploads_wait()
        blk.close()
    for f in (ff, ffu, ffq):
        f.close()
    pin.close()
    pdep.close()


# ------------------------------------------------------------------ 2. maps
_SEQ = {}


def _sequence(api, synth, size, n=12):
    """(cam, frames): frames = (t, colour rgb [H,W,3], grey of it under the default weights, depth, pose, ref)"""
    if size not in _SEQ:
        w, h = size
        cam = synth.TINY if size == (160, 96) else synth.Camera(w, h, 200.0, 200.0, (w - 1) / 2, (h - 1) / 2)
        frames = []
        for t, img, dep, pose, ref in synth.sequence(cam, synth.Scene(), n, keyframe_every=4):
            rgb = cc.colorize(img, t)
            frames.append((t, rgb, api.gray_from_color(rgb, "rgb8"), dep, pose, ref))
        _SEQ[size] = (cam, frames)
    return _SEQ[size]


def _run_form(api, cam, form, enc, images, frames):
    """the sequence through one form; images[i]: frame i's image in `enc` ('mono8': grey).  -> (labels, seeds, map)"""
    n = len(frames)
    fmt = api.frame_format(enc)
    color = None if enc == "mono8" else enc
    refs = np.array([f[5] for f in frames], np.int32)
    poses = [f[4] for f in frames]
    deps = [f[3] for f in frames]
    if form == "live":
        ff = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=1 << 18, flags=api.DSM_FLAG_UPLOAD_STREAM)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        for t in range(n):
            ff.frame_upload_fmt(t & 1, images[t], deps[t], fmt)
            ff.fuse_frame_resident(t & 1, int(refs[t]), poses[t])
        out = (ff.labels(), ff.seeds(), ff.map_download())
        ff.close()
        return out
    if form == "batch":
        hs = [api.FusionFunctions.from_camera(cam, frame_slots=n, surfel_capacity=1 << 18, pipeline_depth=1) for _ in range(8)]
        pin = api.PinnedFrames(hs[0], n, image_format=color)
        pin.set_many(0, images, deps)
        for hnd in hs:
            hnd.map_upload(np.zeros(0, api.SURFEL_DTYPE))
            hnd.frames_upload_async(0, pin, 0, n)
        batch = api.Batch(hs)
        pl = api.FusionFunctions.pack_replay(list(range(n)), refs, poses)
        s_, r_, p_, m = api.Batch.pack([pl] * 8)
        batch.replay_enqueue(s_, r_, p_, m)
        batch.synchronize()
        out = (hs[0].labels(), hs[0].seeds(), hs[0].map_download())
        last = hs[-1].map_download()
        assert _canon(last) == _canon(out[2]), "handles of one batch disagree"
        for hnd in hs:
            hnd.frame_uploads_wait()
        batch.close()
        for hnd in hs:
            hnd.close()
        pin.close()
        return out
    ff = api.FusionFunctions.from_camera(cam, frame_slots=max(8, n), surfel_capacity=1 << 18, pipeline_depth=8)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    pin = api.PinnedFrames(ff, n, image_format=color)
    pin.set_many(0, images, deps)
    pc = np.stack([api.pose_to_colmajor(p) for p in poses])
    if form == "group":  # asynchronous uploads, then one enqueue: groups of four frames
        ff.frames_upload_async(0, pin, 0, n)
        s_, r_, p_ = ff.pack_replay(list(range(n)), refs, poses)
        ff.replay_enqueue(s_, r_, p_)
    else:  # "enqueue_host": each group converted on the stream that runs its superpixel stages
        ff.replay_enqueue_host(pin, 0, refs[:8], pc[:8])
        ff.replay_enqueue_host(pin, 8, refs[8:], pc[8:])
    out = (ff.labels(), ff.seeds(), ff.map_download())
    ff.frame_uploads_wait()
    ff.close()
    pin.close()
    return out


@pytest.mark.parametrize("form", ["live", "batch", "group", "enqueue_host"])
@pytest.mark.parametrize("size", [(160, 96), (250, 263)], ids=["160x96", "250x263"])
def test_maps_from_colour_frames(mods, size, form):
    api, synth, ob = mods
    cam, frames = _sequence(api, synth, size)
    enc = {"live": "rgb8", "batch": "bgra8", "group": "bgr8", "enqueue_host": "rgba8"}[form]
    grey = [f[2] for f in frames]
    for f in frames:  # the channels genuinely differ: a channel-order bug changes the grey of most pixels
        assert (api.gray_from_color(f[1][..., ::-1], "rgb8") != f[2]).mean() > 0.5
    want = _run_form(api, cam, form, "mono8", grey, frames)
    got = _run_form(api, cam, form, enc, [cc.to_encoding(f[1], enc) for f in frames], frames)
    # (a frame has (w / 8) * (h / 8) superpixels, each a candidate surfel: a quarter of ONE frame's worth is a floor that a working
    # sequence of twelve frames cannot miss and an empty or degenerate one cannot reach)
    assert len(want[2]) > (cam.width // 8) * (cam.height // 8) // 4, "the sequence fused next to nothing"
    assert np.array_equal(got[0], want[0]), "labels"
    assert not fields_equal(got[1], want[1]), "seed table"
    assert _canon(got[2]) == _canon(want[2]), "map"
    if form == "live":
        orc = ob.PortOracle(cam)
        lo = np.zeros(0, ob.SURFEL_DTYPE)
        for (t, rgb, g, dep, pose, ref) in frames:
            lo, ko = orc.fuse_map(ref, g, dep, pose, lo)
        assert not fields_equal(got[2], lo.astype(api.SURFEL_DTYPE)), "colour path vs PortOracle on the grey frames"
        assert np.array_equal(got[0], orc.labels())


# ------------------------------------------------------------------ 3. colour + uint16 depth in one call
def test_colour_and_u16_depth_in_one_call(mods):
    api, synth, ob = mods
    w, h = 250, 263
    cam = synth.Camera(w, h, 200.0, 200.0, (w - 1) / 2, (h - 1) / 2, far=6.0, near=0.3, rgbd=True)
    rng = np.random.default_rng(11)
    rgb = _exhaustive(w, h)
    u16 = [rng.integers(0, 65536, (h, w)).astype(np.uint16) for _ in range(S)]
    ref = api.FusionFunctions.from_camera(cam, frame_slots=S, surfel_capacity=1 << 16)
    for enc, weights, (scale, op) in (("bgr8", cc.PRESETS["opencv15"], (5000.0, "divide")), ("rgba8", cc.CUSTOM, (0.001, "multiply"))):
        col = [cc.to_encoding(rgb[i], enc) for i in range(S)]
        for i in range(S):
            ref.frame_upload(i, api.gray_from_color(col[i], enc, weights), api.depth_from_u16(u16[i], scale, op))
        want = [ref.frame(i) for i in range(S)]
        fmt = api.frame_format(enc, weights, (scale, op))

        def check(f, form):
            for i in range(S):
                gi, gd = f.frame(i)
                assert np.array_equal(gi, want[i][0]), f"{enc} {form}: image {i}"
                assert np.array_equal(gd.view(np.uint32), want[i][1].view(np.uint32)), f"{enc} {form}: depth {i}"

        ff = api.FusionFunctions.from_camera(cam, frame_slots=S, surfel_capacity=1 << 18, pipeline_depth=4)
        ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
        for i in range(S):
            ff.frame_upload_fmt(i, col[i], u16[i], fmt)
        check(ff, "sync")
        pin = api.PinnedFrames(ff, S, depth_u16=(scale, op), image_format=enc, gray_weights=weights)
        assert pin.depth(0).dtype == np.uint16 and pin.image(0).shape == (h, w, cc.CHANNELS[enc])
        pin.set_many(0, col, u16)
        for i in range(S):
            ff.frame_upload_fmt(i, col[(i + 1) % S], u16[(i + 1) % S], fmt)  # (other contents first)
        ff.frames_upload_async(0, pin, 0, S)
        check(ff, "async")
        ff.frame_uploads_wait()
        for i in range(S):
            ff.frame_upload_fmt(i, col[(i + 1) % S], u16[(i + 1) % S], fmt)
        ff.replay_enqueue_host(pin, 0, np.zeros(S, np.int32), np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (S, 1)))
        check(ff, "enqueue_host")
        # mono8 through the descriptor: what the plain and the *_u16 calls do
        g0 = api.gray_from_color(col[0], enc, weights)
        ff.frame_upload_fmt(1, g0, u16[0], api.frame_format("mono8", None, (scale, op)))
        ff.frame_upload_fmt(2, g0, want[0][1], api.frame_format())
        for s in (1, 2):
            gi, gd = ff.frame(s)
            assert np.array_equal(gi, want[0][0]) and np.array_equal(gd.view(np.uint32), want[0][1].view(np.uint32)), f"mono8 slot {s}"
        ff.close()
        pin.close()
    ref.close()


# ------------------------------------------------------------------ 4. the node
@pytest.mark.parametrize("enc,u16", [("rgb8", False), ("bgra8", True)])
def test_node_image_input_color(mods, tmp_path, enc, u16):
    """a short keyframe circuit fed with image_input_color (and depth_input or depth_input_u16) and with the grey frames: snapshot
    digest and saved cloud equal; the plain image_input still refuses colour"""
    api, synth, ob = mods
    import node_state
    from densesurfelmapping_amd import surfel_map
    cam = synth.NODE_CAM_RGBD
    scene = synth.Scene(seed=5, tum=True, frames_per_period=16, intensity_noise=8.0, checker=25.0, n_boxes=6)
    weights = cc.PRESETS["opencv15"] if u16 else None
    rendered, colour = {}, {}
    for tl in range(16):
        img, d16 = synth.render_u16(cam, scene, tl)[:2]
        colour[tl] = cc.to_encoding(cc.colorize(img, tl), enc)
        rendered[tl] = (api.gray_from_color(colour[tl], enc, weights), d16 if u16 else api.depth_from_u16(d16, 5000.0))
    assert (api.gray_from_color(colour[0][..., [2, 1, 0] + ([3] if cc.CHANNELS[enc] == 4 else [])], enc, weights) != rendered[0][0]).mean() > 0.5
    out = {}
    for use_color in (True, False):
        node = surfel_map.SurfelMap(cam, drift_free_poses=3)
        t = 0
        for ev in synth.node_messages(cam, scene, 22, lap=16, keyframe_every=4, drift_rate=0.1, frames=rendered):
            if ev[0] == "image":
                if use_color:
                    if t == 0:
                        with pytest.raises(api.DsmError) as e:
                            node.image_input(ev[1], colour[0][..., 0], encoding="bgr8")
                        assert e.value.code == api.DSM_E_INVALID
                    node.image_input_color(ev[1], colour[t % 16], enc, weights)
                else:
                    node.feed(ev)
                t += 1
            elif ev[0] == "depth" and u16:
                node.depth_input_u16(ev[1], ev[2], 5000.0, "divide")
            else:
                node.feed(ev)
        assert node.frames_fused == 22
        path = str(tmp_path / f"cloud_{int(use_color)}.pcd")
        node.save_cloud(path)
        out[use_color] = (node_state.digest(node_state.snapshot(node)), node_state.file_digest(path)["sha256"], len(node.local_surfels()))
        node.close()
    # (only the surfels of the last few keyframes are local, and a keyframe's 1200 superpixels are not all valid: an eighth of one
    # frame's worth is a floor a working node cannot miss and an empty one cannot reach)
    assert out[True][2] > (cam.width // 8) * (cam.height // 8) // 8, "the log fused next to nothing"
    assert out[True][0] == out[False][0], "node state"
    assert out[True][1] == out[False][1], "saved cloud"


# ------------------------------------------------------------------ 5. arguments
def test_fmt_arguments_refused(mods):
    """bad weights / shift / format / step / struct_size: DSM_E_INVALID before any device work; the handle still works afterwards"""
    api, synth, ob = mods
    from densesurfelmapping_amd import surfel_map
    lib = api.load_library()
    cam = synth.TINY
    w, h = cam.width, cam.height
    ff = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=1 << 16, pipeline_depth=1)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    rng = np.random.default_rng(2)
    col = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    dep = np.ones((h, w), np.float32)
    pin = api.PinnedFrames(ff, 2, image_format="rgb8")
    H = ff._h
    vp = C.c_void_p
    P = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (2, 1))
    refs = np.zeros(2, np.int32)
    pi, pd = pin.image(0), pin.depth(0)
    B = C.byref
    calls = {
        "sync": lambda f, st=3 * w: lib.dsm_frame_upload_fmt(H, 0, P(col), st, P(dep), 4 * w, B(f) if f else None),
        "device": lambda f, st=3 * w: lib.dsm_frame_upload_device_fmt(H, 0, P(col), st, P(dep), 4 * w, B(f) if f else None),
        "async": lambda f, st=pi.strides[0]: lib.dsm_frame_upload_async_fmt(H, 0, P(pi), st, P(pd), pd.strides[0], B(f) if f else None),
        "async_n": lambda f, st=pi.strides[0]: lib.dsm_frames_upload_async_fmt(H, 0, 2, P(pi), st, pin._bytes_img, P(pd), pd.strides[0], pin._bytes_dep,
                                                                              B(f) if f else None),
        "enqueue_host": lambda f, st=pi.strides[0]: lib.dsm_replay_enqueue_host_fmt(H, 2, P(pi), st, pin._bytes_img, P(pd), pd.strides[0], pin._bytes_dep,
                                                                                   P(refs), P(eye), None, B(f) if f else None),
    }

    def fmt(**kw):
        f = api.frame_format("rgb8")
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    bad = {"negative weight": fmt(gray_wb=-1), "shift 0": fmt(gray_shift=0), "shift 23": fmt(gray_shift=23, gray_wr=1, gray_wg=1, gray_wb=1),
           "sum above 1 << shift": fmt(gray_wr=4900), "unknown image format": fmt(image_format=5), "negative image format": fmt(image_format=-1),
           "unknown depth format": fmt(depth_format=2), "struct_size": fmt(struct_size=32), "struct_size 0": fmt(struct_size=0),
           "u16 scale": fmt(depth_format=api.DEPTH_U16, depth_scale=0.0), "null": None}
    for name, call in calls.items():
        for what, f in bad.items():
            assert call(f) == api.DSM_E_INVALID, (name, what)
        assert call(fmt(), st=3 * w - 1) == api.DSM_E_INVALID, (name, "step below channels * w")
        assert call(fmt(image_format=api.IMAGE_RGBA8), st=4 * w - 1) == api.DSM_E_INVALID, (name, "step below 4 * w")
    # nothing went to the device: the handle is clean and still works
    ff.frame_upload_fmt(0, col, dep, api.frame_format("rgb8"))
    assert np.array_equal(ff.frame(0)[0], api.gray_from_color(col, "rgb8"))
    assert np.array_equal(ff.frame(0)[1], dep)
    ff.close()
    pin.close()
    node = surfel_map.SurfelMap(cam, drift_free_poses=3)
    for enc, wts, a in (("mono16", None, col), ("mono8", None, col), ("rgb8", (-1, 1, 1, 8), col), ("rgb8", (1, 1, 1, 0), col), ("rgb8", (1, 1, 1, 23), col),
                        ("rgb8", (200, 50, 7, 8), col), ("rgba8", None, col)):  # (the last: rows of 3 * w bytes are shorter than 4 * w)
        with pytest.raises(api.DsmError) as e:
            node.image_input_color((1000, 0), a, enc, wts)
        assert e.value.code == api.DSM_E_INVALID, (enc, wts)
    with pytest.raises(api.DsmError) as e:
        node.image_input((1000, 0), col[..., 0], encoding="bgr8")
    assert e.value.code == api.DSM_E_INVALID
    node.image_input_color((1000, 0), col, "rgb8")  # still usable
    node.close()
