"""Colour camera frames converted on the device against the host conversion, on one box, in alternating runs (include/dsm.h,
dsm_frame_format and the *_fmt entry points).

    python tools/bench_image_color.py [--reps 2] [--frames 3000] [--only device|host|mono8] [--encoding rgb8] [--out FILE]

One streamed sequence through replay.HipEngine (dsm_replay_enqueue_host[_fmt], frame groups of pipeline depth 24, frames packed
into page-locked blocks on a prefetch thread) at 640x480, the TUM-style RGB-D configuration, float depth:

  device  (a) the source yields the camera's colour frames; they are packed and streamed at 3 (4) bytes a pixel and converted to
          grey on the device (HipEngine(image_format=...))
  host    (b) the same colour frames converted to grey by the host on the prefetch thread, frame by frame (what a caller of the
          mono8 entry points has to do), then streamed as mono8 -- the conversion is counted.  It is the fixed-point sum in numpy
          uint32 arithmetic (one thread); it is checked against api.gray_from_color before the run
  mono8   (c) grey frames that exist already, streamed as mono8: the ceiling

The colour frames are rendered once (a loop of `--period` frames).  All three sides fuse the same maps.  One JSON object per run is
printed, then a summary.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_gray(image, swap, weights):
    """the device's arithmetic on the host, as fast as plain numpy does it: uint32 multiply-adds, one pass per channel"""
    wr, wg, wb, shift = weights
    r, b = (image[..., 2], image[..., 0]) if swap else (image[..., 0], image[..., 2])
    acc = r.astype(np.uint32) * np.uint32(wr)
    acc += image[..., 1].astype(np.uint32) * np.uint32(wg)
    acc += b.astype(np.uint32) * np.uint32(wb)
    acc += np.uint32(1 << (shift - 1))
    acc >>= np.uint32(shift)
    return acc.astype(np.uint8)


class _Loop:
    """frames() of a pre-rendered loop of (colour, grey, depth): side 'device' yields the colour frame, 'host' converts it there
    and then, 'mono8' yields the grey frame that exists already"""

    def __init__(self, scene, frames, side, swap, weights):
        self.scene, self.f, self.side, self.swap, self.weights = scene, frames, side, swap, weights
        self.host_seconds = 0.0

    def frames(self, a, b):
        for t in range(a, b):
            col, grey, dep = self.f[t % len(self.f)]
            if self.side == "device":
                img = col
            elif self.side == "host":
                t0 = time.perf_counter()
                img = host_gray(col, self.swap, self.weights)
                self.host_seconds += time.perf_counter() - t0
            else:
                img = grey
            yield img, dep, self.scene.pose(t)


def sequence(api, replay, cam, scene, frames, side, encoding, weights, n):
    eng = replay.HipEngine(cam, capacity=1 << 21, image_format=encoding if side == "device" else None, gray_weights=weights)
    src = _Loop(scene, frames, side, encoding.startswith("bgr"), weights)
    eng.replay(src, 0, 480)  # warm-up (graph captures, page-locked blocks)
    src.host_seconds = 0.0
    eng.replay(src, 480, 480 + n, origin=0)
    st = dict(eng.stats)
    size = eng.ff.map_size()
    eng.close()
    fps = st["frames"] / st["seconds"]
    return {"frames_per_s": round(fps, 1), "bytes_per_frame": st["bytes_per_frame"], "link_GBps": round(fps * st["bytes_per_frame"] / 1e9, 3),
            "host_conversion_ms_per_frame": round(src.host_seconds / n * 1e3, 4), "live_surfels": int(size)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--only", choices=("device", "host", "mono8"), default=None, help="one side only (a profiler run)")
    ap.add_argument("--encoding", default="rgb8", choices=("rgb8", "bgr8", "rgba8", "bgra8"))
    ap.add_argument("--period", type=int, default=32, help="frames of the rendered loop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import color_cases as cc
    from densesurfelmapping_amd import api, replay, synth
    cam = synth.VGA_RGBD
    scene = synth.Scene(seed=7, tum=True, frames_per_period=100, intensity_noise=8.0, checker=25.0, n_boxes=6)
    weights = api.GRAY_OPENCV_14BIT
    frames = []
    for t in range(args.period):
        img, dep, _ = synth.render(cam, scene, t)
        col = cc.to_encoding(cc.colorize(img, t), args.encoding)
        grey = api.gray_from_color(col, args.encoding, weights)
        assert np.array_equal(host_gray(col, args.encoding.startswith("bgr"), weights), grey)
        frames.append((col, grey, dep))
    sides = [args.only] if args.only else ["device", "host", "mono8"]
    runs = []
    for rep in range(args.reps):
        for side in (sides if rep % 2 == 0 else sides[::-1]):  # alternating: a b c c b a ...
            r = {"leg": "one_streamed_sequence", "scene": "tum640_" + args.encoding, "side": side, "rep": rep,
                 **sequence(api, replay, cam, scene, frames, side, args.encoding, weights, args.frames)}
            print(json.dumps(r), flush=True)
            runs.append(r)
    summary = {}
    for r in runs:
        summary.setdefault(r["side"], []).append(r["frames_per_s"])
    assert len({r["live_surfels"] for r in runs}) == 1, "the sides fused different maps"
    rec = {"device": torch.cuda.get_device_name(0), "runs": runs, "frames_per_s": summary}
    print(json.dumps({"summary": summary}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
