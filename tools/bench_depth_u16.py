"""f32 against sensor-native u16 depth on one box, in alternating runs (include/dsm.h, the *_u16 entry points).

    python tools/bench_depth_u16.py [--reps 2] [--legs streamed,sequence,live] [--only u16|f32] [--out FILE]

  streamed  bench.py's `streamed_input` form: 128 subsequences in 4 batches of 32 (one host thread each), chunks of 16 frames
            double-buffered from page-locked memory (dsm_frames_upload_async[_u16]), maps resident -- at 1226x370 with
            KITTI-style u16 / 256 depth and at 640x480 TUM (u16 / 5000)
  sequence  one streamed sequence through replay.HipEngine (dsm_replay_enqueue_host[_u16], frame groups of pipeline depth 24,
            frames packed on a prefetch thread) at 1226x370
  live      the 640x480 live callback: per frame upload into one of two slots, one graph replay, wait -- the f32 side pays the
            host conversion (u16 / 5000 in numpy) that a caller of the float upload does; p50 / p99 of the frame latency

Frames are rendered once per scene (a loop of `--period` frames) and quantised as the sensor stores them; the f32 runs get exactly
the host conversion of the same u16 frames, so both sides fuse the same maps.  One JSON object per run is printed, then a summary.
"""
import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scenes(synth, api, period):
    """name -> (camera, [(image, u16)], scale, poses): KITTI-style 1226x370 drive (u16 = round(metres x 256)), TUM 640x480 room"""
    out = {}
    cam, scene = synth.KITTI_1226, synth.Scene()
    fr = []
    for t in range(period):
        img, dep, _ = synth.render(cam, scene, t)
        fr.append((img, np.clip(np.round(dep.astype(np.float64) * 256.0), 0, 65535).astype(np.uint16)))
    out["kitti1226_u16_256"] = (cam, scene, fr, 256.0)
    cam, scene = synth.VGA_RGBD, synth.Scene(seed=7, tum=True, frames_per_period=100, intensity_noise=8.0, checker=25.0, n_boxes=6)
    out["tum640_u16_5000"] = (cam, scene, [synth.render_u16(cam, scene, t)[:2] for t in range(period)], 5000.0)
    return out


def streamed(api, cam, scene, frames, scale, u16, B=128, n_bat=4, C=16, warm_chunks=6, chunks=24):
    period = len(frames)
    hs = [api.FusionFunctions.from_camera(cam, frame_slots=2 * C, surfel_capacity=1 << 20, pipeline_depth=1) for _ in range(B)]
    pf = api.PinnedFrames(hs[0], period, depth_u16=(scale, "divide") if u16 else None)
    for i, (img, d16) in enumerate(frames):
        pf.set(i, img, d16 if u16 else api.depth_from_u16(d16, scale))
    for h in hs:
        h.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    per = B // n_bat
    groups = [list(range(g * per, (g + 1) * per)) for g in range(n_bat)]
    bts = [api.Batch([hs[b] for b in grp]) for grp in groups]
    phase = [(b * 7) % period for b in range(B)]
    poses = [api.pose_to_colmajor(scene.pose(t)) for t in range(period)]

    def send(g, k):
        for b in groups[g]:
            i = 0
            while i < C:
                t = (k * C + i + phase[b]) % period
                n = min(C - i, period - t)
                hs[b].frames_upload_async((k & 1) * C + i, pf, t, n)
                i += n

    def plan(b, k):
        ts = [(k * C + i + phase[b]) % period for i in range(C)]
        return (np.ascontiguousarray([(k & 1) * C + i for i in range(C)], np.int32),
                np.ascontiguousarray([(k * C + i) // 5 for i in range(C)], np.int32), np.stack([poses[t] for t in ts]))

    def run(g, k0, k1, total):
        for k in range(k0, k1):
            if k + 1 < total:
                send(g, k + 1)
            s, r, p, n = api.Batch.pack([plan(b, k) for b in groups[g]])
            bts[g].replay_enqueue(s, r, p, n)

    total = warm_chunks + chunks
    pool = cf.ThreadPoolExecutor(n_bat)
    for g in range(n_bat):
        send(g, 0)
    list(pool.map(lambda g: run(g, 0, warm_chunks, total), range(n_bat)))
    for bt in bts:
        bt.synchronize()
    t0 = time.perf_counter()
    list(pool.map(lambda g: run(g, warm_chunks, total, total), range(n_bat)))
    for bt in bts:
        bt.synchronize()
    dt = time.perf_counter() - t0
    fps = B * chunks * C / dt
    frame_bytes = pf.pitch * cam.height * (3 if u16 else 5)
    res = {"frames_per_s": round(fps, 1), "link_GBps": round(fps * frame_bytes / 1e9, 2), "bytes_per_frame": frame_bytes,
           "mean_live_surfels": round(float(np.mean([h.map_size() for h in hs[:8]])))}
    for bt in bts:
        bt.close()
    for h in hs:
        h.frame_uploads_wait()
        h.close()
    pf.close()
    pool.shutdown()
    return res


class _Loop:
    """frames() of a pre-rendered loop: uint16, or its host conversion"""

    def __init__(self, api, scene, frames, scale, u16):
        self.api, self.scene, self.f, self.scale, self.u16 = api, scene, frames, scale, u16
        self.conv = None if u16 else [api.depth_from_u16(d, scale) for _, d in frames]

    def frames(self, a, b):
        for t in range(a, b):
            i = t % len(self.f)
            yield self.f[i][0], (self.f[i][1] if self.u16 else self.conv[i]), self.scene.pose(t)


def sequence(api, replay, cam, scene, frames, scale, u16, n=3000):
    eng = replay.HipEngine(cam, capacity=1 << 21, depth_u16=(scale, "divide") if u16 else None)
    src = _Loop(api, scene, frames, scale, u16)
    eng.replay(src, 0, 480)  # warm-up (graph captures, page-locked blocks)
    eng.replay(src, 480, 480 + n, origin=0)
    st = dict(eng.stats)
    eng.close()
    return {"frames_per_s": round(st["frames"] / st["seconds"], 1), "bytes_per_frame": st["bytes_per_frame"]}


def live(api, cam, scene, frames, scale, u16, n=300):
    ff = api.FusionFunctions.from_camera(cam, frame_slots=2, surfel_capacity=1 << 19)
    ff.map_upload(np.zeros(0, api.SURFEL_DTYPE))
    lat = []
    for t in range(n + 20):
        img, d16 = frames[t % len(frames)]
        pose = scene.pose(t)
        t0 = time.perf_counter()
        if u16:
            ff.frame_upload_u16(t & 1, img, d16, scale, "divide")
        else:
            ff.frame_upload(t & 1, img, api.depth_from_u16(d16, scale))  # the caller's conversion on the callback thread
        ff.fuse_frame_resident(t & 1, t // 4, pose)
        ff.synchronize()
        if t >= 20:
            lat.append(time.perf_counter() - t0)
    ff.close()
    lat = np.array(lat) * 1e3
    return {"p50_ms": round(float(np.percentile(lat, 50)), 3), "p99_ms": round(float(np.percentile(lat, 99)), 3),
            "frames_per_s": round(len(lat) / (lat.sum() / 1e3), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--legs", default="streamed,sequence,live")
    ap.add_argument("--only", choices=("u16", "f32"), default=None, help="one side only (a profiler run)")
    ap.add_argument("--period", type=int, default=32, help="frames of the rendered loop per scene")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from densesurfelmapping_amd import api, replay, synth
    legs = args.legs.split(",")
    sc = scenes(synth, api, args.period)
    sides = [args.only == "u16"] if args.only else [False, True]
    runs = []
    for rep in range(args.reps):
        for u16 in (sides if rep % 2 == 0 else sides[::-1]):  # alternating: f32 u16 u16 f32 ...
            side = "u16" if u16 else "f32"
            if "streamed" in legs:
                for name in ("kitti1226_u16_256", "tum640_u16_5000"):
                    cam, scene, fr, scale = sc[name]
                    r = {"leg": "streamed_input", "scene": name, "side": side, "rep": rep, **streamed(api, cam, scene, fr, scale, u16)}
                    print(json.dumps(r), flush=True)
                    runs.append(r)
            if "sequence" in legs:
                cam, scene, fr, scale = sc["kitti1226_u16_256"]
                r = {"leg": "one_streamed_sequence", "scene": "kitti1226_u16_256", "side": side, "rep": rep,
                     **sequence(api, replay, cam, scene, fr, scale, u16)}
                print(json.dumps(r), flush=True)
                runs.append(r)
            if "live" in legs:
                cam, scene, fr, scale = sc["tum640_u16_5000"]
                r = {"leg": "live_callback", "scene": "tum640_u16_5000", "side": side, "rep": rep, **live(api, cam, scene, fr, scale, u16)}
                print(json.dumps(r), flush=True)
                runs.append(r)
    summary = {}
    for r in runs:
        key = f"{r['leg']}/{r['scene']}/{r['side']}"
        summary.setdefault(key, []).append(r.get("frames_per_s"))
    rec = {"device": torch.cuda.get_device_name(0), "runs": runs, "frames_per_s": summary}
    print(json.dumps({"summary": summary}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
