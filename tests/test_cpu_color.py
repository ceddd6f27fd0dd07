"""CPU side of the colour image input: the host reference of the device conversion (api.gray_from_color), the presets, the format
descriptor, and the host code of the *_fmt family (dsm_host_pack_frames_fmt, dsm_frame_format_init)."""
import ctypes as C
import os

import numpy as np
import pytest

import color_cases as cc


@pytest.fixture(scope="module")
def api():
    from densesurfelmapping_amd import api, build
    build.build_library()
    return api


def test_presets_are_the_headers(api):
    hdr = open(os.path.join(os.path.dirname(api.__file__), "..", "include", "dsm.h")).read()
    for name, w in (("DSM_GRAY_OPENCV_14BIT", api.GRAY_OPENCV_14BIT), ("DSM_GRAY_OPENCV_15BIT", api.GRAY_OPENCV_15BIT), ("DSM_GRAY_PIL_L", api.GRAY_PIL_L)):
        assert "#define %s {%d, %d, %d, %d}" % ((name,) + tuple(w)) in hdr, name
        assert tuple(w) in cc.PRESETS.values()
    for i, name in enumerate(("MONO8", "RGB8", "BGR8", "RGBA8", "BGRA8")):
        assert "#define DSM_IMAGE_%s %d\n" % (name, i) in hdr and getattr(api, "IMAGE_" + name) == i
    assert "#define DSM_DEPTH_F32 0\n" in hdr and "#define DSM_DEPTH_U16 1\n" in hdr
    assert "#define DSM_ABI_VERSION 4 " in hdr
    for s in ("dsm_frame_format_init", "dsm_frame_upload_fmt", "dsm_frame_upload_device_fmt", "dsm_frame_upload_async_fmt",
              "dsm_frames_upload_async_fmt", "dsm_replay_enqueue_host_fmt", "dsm_host_pack_frames_fmt"):
        assert s in api.ABI_SYMBOLS and s + "(" in hdr
    from densesurfelmapping_amd import surfel_map
    assert "dsm_surfel_map_image_input_color" in surfel_map.ABI_SYMBOLS


def test_pil_l_preset_is_pillows_convert_l(api):
    """DSM_GRAY_PIL_L against the real thing: all 65 536 (r, g) pairs at b = 0 and b = 255, and a million random triples"""
    Image = pytest.importorskip("PIL.Image")
    r, g = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rng = np.random.default_rng(0)
    cases = [np.stack([r, g, np.full_like(r, b)], axis=-1) for b in (0, 255)] + [rng.integers(0, 256, (1000, 1000, 3), dtype=np.uint8)]
    for k, rgb in enumerate(cases):
        want = np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
        got = api.gray_from_color(rgb, "rgb8", api.GRAY_PIL_L)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (k, int((got != want).sum()))


@pytest.mark.parametrize("name", sorted(cc.PRESETS))
def test_presets_keep_grey_and_add_up(api, name):
    wr, wg, wb, shift = cc.PRESETS[name]
    assert wr + wg + wb == 1 << shift
    v = np.arange(256, dtype=np.uint8)
    for enc in cc.ENCODINGS:
        assert np.array_equal(api.gray_from_color(cc.to_encoding(np.stack([v, v, v], axis=-1), enc), enc, cc.PRESETS[name]), v), enc
    assert np.array_equal(api.gray_from_color(np.stack([v, v, v], axis=-1), "rgb8"), v), "default weights"


@pytest.mark.parametrize("name", sorted(cc.WEIGHT_SETS))
def test_channel_order_and_alpha(api, name):
    """rgb8 against bgr8 with R and B swapped give equal output; alpha has no effect; the formula itself, pixel by pixel"""
    w = cc.WEIGHT_SETS[name]
    rgb = cc.exhaustive_rgb(64, 64, seed=3)
    rng = np.random.default_rng(4)
    want = api.gray_from_color(rgb, "rgb8", w)
    wr, wg, wb, shift = w
    flat = rgb.reshape(-1, 3).tolist()
    assert want.ravel().tolist() == [(r * wr + g * wg + b * wb + (1 << (shift - 1))) >> shift for r, g, b in flat]
    assert np.array_equal(api.gray_from_color(rgb[..., ::-1], "bgr8", w), want)
    for enc in ("rgba8", "bgra8"):
        for alpha in (None, np.zeros((64, 64), np.uint8), rng.integers(0, 256, (64, 64), dtype=np.uint8)):
            assert np.array_equal(api.gray_from_color(cc.to_encoding(rgb, enc, alpha), enc, w), want), enc
    # the channels matter: reading rgb8 as bgr8 changes the grey (a channel-order bug cannot hide)
    assert (api.gray_from_color(rgb, "bgr8", w) != want).mean() > 0.5
    for bad in ((-1, 1, 1, 8), (1, 1, 1, 0), (1, 1, 1, 23), (200, 50, 7, 8)):
        with pytest.raises(ValueError):
            api.gray_from_color(rgb, "rgb8", bad)
    with pytest.raises(ValueError):
        api.gray_from_color(rgb, "rgba8", w)
    with pytest.raises(ValueError):
        api.gray_from_color(rgb[..., 0], "mono8", w)


def test_frame_format_init_and_struct(api):
    lib = api.load_library()
    f = api._FrameFormat()
    lib.dsm_frame_format_init(C.byref(f))
    assert C.sizeof(api._FrameFormat) == 36 == f.struct_size
    assert (f.image_format, f.gray_wr, f.gray_wg, f.gray_wb, f.gray_shift, f.depth_format, f.depth_scale, f.depth_op) == \
        (api.IMAGE_MONO8,) + api.GRAY_OPENCV_14BIT + (api.DEPTH_F32, 1.0, api.DEPTH_U16_DIVIDE)
    g = api.frame_format()
    assert bytes(f) == bytes(g)
    g = api.frame_format("bgra8", api.GRAY_PIL_L, (5000.0, "divide"))
    assert (g.image_format, g.gray_shift, g.depth_format, g.depth_scale) == (api.IMAGE_BGRA8, 16, api.DEPTH_U16, 5000.0)
    lib.dsm_abi_version.restype = C.c_int
    assert lib.dsm_abi_version() == 4


@pytest.mark.parametrize("enc,u16", [("rgb8", False), ("bgra8", True), ("mono8", True), ("mono8", False)])
def test_host_pack_frames_fmt(api, enc, u16):
    """dsm_host_pack_frames_fmt (host code only): colour rows -- contiguous and strided -- land in the slot layout at channels x
    pitch bytes a row, depth rows at 4 or 2 bytes a pixel, pad bytes untouched; bad steps, formats and null planes are refused."""
    lib = api.load_library()
    rng = np.random.default_rng(1)
    n, w, h = 5, 166, 103
    ch = api.image_channels(enc)
    ddt = np.uint16 if u16 else np.float32
    de = np.dtype(ddt).itemsize
    pitch, ch_, bi, bd = api.PinnedFrames.layout(h, w, depth_u16=(1.0, "divide") if u16 else None, image_format=enc)
    assert (pitch, ch_, bi, bd) == (192, ch, 192 * h * ch, 192 * h * de)
    wide_i = rng.integers(0, 256, (h, (w + 9) * ch + 1), dtype=np.uint8)
    last = np.lib.stride_tricks.as_strided(wide_i[:, 3:], shape=(h, w, ch), strides=(wide_i.strides[0], ch, 1))
    ims = [rng.integers(0, 256, (h, w, ch), dtype=np.uint8) for _ in range(n - 1)] + [last]
    wide_d = rng.integers(0, 60000, (h, w + 5)).astype(ddt)
    dps = [rng.integers(0, 60000, (h, w)).astype(ddt) for _ in range(n - 1)] + [wide_d[:, 2:2 + w]]
    dst_i, dst_d = np.full((n, h, pitch * ch), 7, np.uint8), np.full((n, h, pitch), 9, ddt)
    fmt = api.frame_format(enc, None, (1.0, "divide") if u16 else None)

    def call(n_, ims_, dps_, img_step=pitch * ch, dep_step=pitch * de, fmt_=fmt):
        ip = (C.c_void_p * len(ims_))(*[a.ctypes.data if a is not None else None for a in ims_])
        dp = (C.c_void_p * len(dps_))(*[a.ctypes.data for a in dps_])
        ist = (C.c_size_t * len(ims_))(*[a.strides[0] if a is not None else 0 for a in ims_])
        dst = (C.c_size_t * len(dps_))(*[a.strides[0] for a in dps_])
        return lib.dsm_host_pack_frames_fmt(n_, w, h, ip, ist, dp, dst, C.c_void_p(dst_i.ctypes.data), img_step, pitch * h * ch,
                                            C.c_void_p(dst_d.ctypes.data), dep_step, pitch * h * de, C.byref(fmt_) if fmt_ is not None else None)
    assert call(n, ims, dps) == 0
    for i in range(n):
        assert np.array_equal(dst_i[i, :, :w * ch], ims[i].reshape(h, w * ch)) and np.array_equal(dst_d[i, :, :w], dps[i]), i
    assert (dst_i[:, :, w * ch:] == 7).all() and (dst_d[:, :, w:] == 9).all(), "pad bytes were written"
    assert call(0, ims, dps) == 0
    assert call(n, ims, dps, img_step=w * ch - 1) == -1 and "row step" in lib.dsm_last_error(None).decode()
    assert call(n, ims, dps, dep_step=w * de - 1) == -1 and "row step" in lib.dsm_last_error(None).decode()
    assert call(n, ims[:-1] + [None], dps) == -1 and "frame 4" in lib.dsm_last_error(None).decode()
    short = [np.lib.stride_tricks.as_strided(ims[0], shape=(h, w, ch), strides=(w * ch - 1, ch, 1))] + ims[1:]
    assert call(n, short, dps) == -1 and "frame 0" in lib.dsm_last_error(None).decode()
    assert call(n, ims, dps, fmt_=None) == -1
    bad = api.frame_format(enc)
    bad.struct_size -= 4
    assert call(n, ims, dps, fmt_=bad) == -1
    bad = api.frame_format(7)
    assert call(n, ims, dps, fmt_=bad) == -1
    bad = api.frame_format(enc)
    bad.depth_format = 2
    assert call(n, ims, dps, fmt_=bad) == -1
