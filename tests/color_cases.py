"""Shared builders of the colour-image tests (test_cpu_color.py, test_gpu_color.py): weight sets, exhaustive frames, colour
frames whose channels genuinely differ, and the layouts a colour image arrives in."""
import numpy as np

ENCODINGS = ("rgb8", "bgr8", "rgba8", "bgra8")
CHANNELS = {"rgb8": 3, "bgr8": 3, "rgba8": 4, "bgra8": 4}
# (wr, wg, wb, shift): the three presets of include/dsm.h and one caller-made set whose sum stays below 1 << shift and whose
# weights put R, G and B in another order of importance than any preset (a swapped pair of weights cannot pass)
PRESETS = {"opencv14": (4899, 9617, 1868, 14), "opencv15": (9798, 19235, 3735, 15), "pil_l": (19595, 38470, 7471, 16)}
CUSTOM = (1100001, 7, 3094295, 22)
WEIGHT_SETS = dict(PRESETS, custom=CUSTOM)


def to_encoding(rgb, encoding, alpha=None):
    """uint8 [..., 3] R, G, B -> the pixel layout of `encoding`; alpha: uint8 [...] for the 4-byte encodings (default 255)"""
    rgb = np.asarray(rgb, np.uint8)
    first3 = rgb[..., ::-1] if encoding.startswith("bgr") else rgb
    if CHANNELS[encoding] == 3:
        return np.ascontiguousarray(first3)
    a = np.full(rgb.shape[:-1], 255, np.uint8) if alpha is None else np.asarray(alpha, np.uint8)
    return np.ascontiguousarray(np.concatenate([first3, a[..., None]], axis=-1))


def exhaustive_rgb(h, w, seed):
    """uint8 [h, w, 3] R, G, B: each channel takes all 256 values against 0, against 255 and against random values in the other two,
    then random triples; shuffled over the frame (h * w >= 2304 + some random ones)"""
    rng = np.random.default_rng(seed)
    v = np.arange(256, dtype=np.uint8)
    rows = []
    for c in range(3):
        for other in (0, 255, None):
            t = np.zeros((256, 3), np.uint8) if other is None else np.full((256, 3), other, np.uint8)
            if other is None:
                t[:] = rng.integers(0, 256, (256, 3), dtype=np.uint8)
            t[:, c] = v
            rows.append(t)
    fixed = np.concatenate(rows)
    n = h * w
    assert n >= len(fixed), "frame too small for the exhaustive set"
    out = np.concatenate([fixed, rng.integers(0, 256, (n - len(fixed), 3), dtype=np.uint8)])
    rng.shuffle(out, axis=0)
    return np.ascontiguousarray(out.reshape(h, w, 3))


def colorize(gray, t=0):
    """a grey image [H,W] -> uint8 [H,W,3] R, G, B whose channels genuinely differ: R keeps the texture, G and B are bent by smooth,
    different ramps (so that the grey of the result still has the scene's structure, and swapping R and B changes it)"""
    g = np.asarray(gray, np.uint8).astype(np.int64)
    h, w = g.shape
    yy, xx = np.mgrid[0:h, 0:w]
    r = np.clip(g + 40 - (xx * 80) // max(w - 1, 1), 0, 255)
    gg = np.clip((g * 3) // 4 + ((yy + 3 * t) % 64), 0, 255)
    b = np.clip(255 - g // 2 - (xx * 60) // max(w - 1, 1), 0, 255)
    return np.stack([r, gg, b], axis=-1).astype(np.uint8)


def strided(img, step_bytes):
    """a view of img [H, W, C] whose rows are step_bytes apart (a copy inside a larger buffer, at offset 0)"""
    h, w, c = img.shape
    assert step_bytes >= w * c
    buf = np.full((h, step_bytes), 0xA5, np.uint8)
    buf[:, : w * c] = img.reshape(h, w * c)
    return np.lib.stride_tricks.as_strided(buf, shape=(h, w, c), strides=(step_bytes, c, 1)), buf
