"""mono8 + float depth -- the planes that go into their slots as they are, past the conversion kernels -- through every upload form
and every source layout the plane-copy plan (csrc/dsm_frame_copy.h) tells apart, read back from the slots with their pad columns
(dsm_debug_frame_planes): payload equal byte for byte, and the pad columns untouched wherever the rows are written one by one:
2-D copies and the repack kernels write `w` elements of a row.  That is every layout of the synchronous and device-memory
uploads, and every layout but rows at the slot pitch of the asynchronous uploads and the frames that come with an enqueue call,
where such rows go up in one piece and take the bytes between them along.

Row steps: the slot pitch, tight, tight + 1 element.  Frame steps of the multi-frame forms: step * h, and step * h + 64 bytes -- the
padded frame step is what reaches the frame-by-frame branches (1-D per frame at the pitch, 2-D per frame otherwise)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 256x256: w == pitch (tight rows ARE pitched rows); 250x263: pitch 256, ragged; 25x24: the narrowest size dsm_create takes
SIZES = [(256, 256), (250, 263), (25, 24)]
S = 4  # frame slots = frames of a case
FRAME_PAD = 64  # bytes between frames in the padded layouts


@pytest.fixture(scope="module")
def mods():
    import torch
    torch.cuda.init()  # torch's HIP runtime first (see __graft_entry__.build)
    from densesurfelmapping_amd import api, synth
    return api, synth


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


@pytest.mark.parametrize("size", SIZES, ids=["256x256", "250x263_ragged", "25x24_narrow"])
def test_mono_f32_every_form_every_layout(mods, size):
    import torch
    api, synth = mods
    lib = api.load_library()
    w, h = size
    cam = synth.Camera(w, h, 200.0, 200.0, (w - 1) / 2, (h - 1) / 2, far=6.0, near=0.3, rgbd=True)
    rng = np.random.default_rng(w)
    img = rng.integers(0, 256, (S, h, w), dtype=np.uint8)
    dep = rng.integers(0, 1 << 32, (S, h, w), dtype=np.uint64).astype(np.uint32)  # any float bit pattern
    dep[:, 0, :4] = np.array([0x7fc00000, 0xffc12345, 0x7f800001, 0xff800000], np.uint32)  # quiet / signalling NaNs, -inf
    assert np.isnan(dep.view(np.float32)).sum() > 3 * S
    ff = api.FusionFunctions.from_camera(cam, frame_slots=S, surfel_capacity=1 << 16)
    ffu = api.FusionFunctions.from_camera(cam, frame_slots=S, surfel_capacity=1 << 16, flags=api.DSM_FLAG_UPLOAD_STREAM)
    ffq = api.FusionFunctions.from_camera(cam, frame_slots=4, surfel_capacity=1 << 16, pipeline_depth=4)
    ffq.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    pitch = ff.frame_pitch()
    assert pitch == (w + 63) // 64 * 64
    steps = [pitch, w, w + 1]  # in elements
    pat_i = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    pat_d = rng.integers(0, 1 << 32, (h, pitch), dtype=np.uint64).astype(np.uint32)
    room = S * (h * (pitch + 1) + FRAME_PAD)
    pin_i = _Pinned(api, room)
    pin_d = _Pinned(api, room * 4)
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (S, 1))
    refs = np.zeros(S, np.int32)
    vp = C.c_void_p

    def prefill(f, slots):
        for s in slots:
            f.frame_planes(s, image=pat_i, depth=pat_d.view(np.float32))

    def check(f, slot, i, pads_kept, form):
        gi, gd = f.frame_planes(slot)
        gd = gd.view(np.uint32)
        bad = int((gi[:, :w] != img[i]).sum())
        assert bad == 0, f"{form}: {bad} image bytes differ, first {np.argwhere(gi[:, :w] != img[i])[:3].tolist()}"
        bad = int((gd[:, :w] != dep[i]).sum())
        assert bad == 0, f"{form}: {bad} depth words differ, first {np.argwhere(gd[:, :w] != dep[i])[:3].tolist()}"
        if pads_kept:
            assert np.array_equal(gi[:, w:], pat_i[:, w:]), f"{form}: image pad bytes were written"
            assert np.array_equal(gd[:, w:], pat_d[:, w:]), f"{form}: depth pad words were written"

    def host_layout(step, pad):
        """the S frames in page-locked memory, rows `step` elements apart and frames step * h elements + pad bytes apart;
        -> (image frame step, [image addresses], depth frame step, [depth addresses])"""
        out = []
        for pin, src, e in ((pin_i, img, 1), (pin_d, dep.view(np.uint8).reshape(S, h, w * 4), 4)):
            fs = step * e * h + pad
            v = np.lib.stride_tricks.as_strided(pin.a, shape=(S, h, w * e), strides=(fs, step * e, 1))
            pin.a[:] = 0x5A
            v[:] = src
            out += [fs, [pin.a.ctypes.data + i * fs for i in range(S)]]
        return out

    for step in steps:
        fsi, ai, fsd, ad = host_layout(step, 0)
        tag = f"{w}x{h} step {step}"
        # synchronous, on the map stream and on an upload stream of the handle's own: frame s into slot s
        for f, fl in ((ff, "sync"), (ffu, "sync upload-stream")):
            prefill(f, range(S))
            for s in range(S):
                assert lib.dsm_frame_upload(f._h, s, vp(ai[s]), step, vp(ad[s]), step * 4) == 0
                check(f, s, s, True, f"{tag} {fl} slot {s}")
        # device memory
        di = torch.from_numpy(pin_i.a.copy()).cuda()
        dd = torch.from_numpy(pin_d.a.copy()).cuda()
        prefill(ff, range(S))
        for s in range(S):
            assert lib.dsm_frame_upload_device(ff._h, s, vp(di.data_ptr() + s * fsi), step, vp(dd.data_ptr() + s * fsd), step * 4) == 0
            check(ff, s, s, True, f"{tag} device slot {s}")
        torch.cuda.synchronize()
        # asynchronous, one frame and S frames; frames that come with the enqueue call (frame f -> slot f mod 4)
        for pad in (0, FRAME_PAD):
            fsi, ai, fsd, ad = host_layout(step, pad)
            ptag = f"{tag} frame pad {pad}"
            prefill(ff, range(S))
            assert lib.dsm_frame_upload_async(ff._h, 3, vp(ai[1]), step, vp(ad[1]), step * 4) == 0
            check(ff, 3, 1, step != pitch, f"{ptag} async single")
            prefill(ff, [3])
            assert lib.dsm_frames_upload_async(ff._h, 0, S, vp(ai[0]), step, fsi, vp(ad[0]), step * 4, fsd) == 0
            for s in range(S):
                check(ff, s, s, step != pitch, f"{ptag} async x{S} slot {s}")
            ff.frame_uploads_wait()
            prefill(ffq, range(S))
            assert lib.dsm_replay_enqueue_host(ffq._h, S, vp(ai[0]), step, fsi, vp(ad[0]), step * 4, fsd,
                                               refs.ctypes.data_as(vp), eye.ctypes.data_as(vp), None) == 0
            for s in range(S):
                check(ffq, s, s, step != pitch, f"{ptag} enqueue_host slot {s}")
            ffq.replay_wait()
    for f in (ff, ffu, ffq):
        f.close()
    pin_i.close()
    pin_d.close()
