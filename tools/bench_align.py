#!/usr/bin/env python
"""Cost of aligning a depth frame to the surfel map (dsm_align_equations, dsm_align_frame) at 640x480 and 1226x370.

  replay   the map a node grows over n_frames frames of the synthetic circuit; the latest frame, still in its slot, is aligned
           against kind ALL from the pose it was fused with
  large    a map of n_large surfels made on the host, spread through the camera's view volume (tools/bench_render.py's); the frame is
           what the map itself shows from the identity pose, the guess is 20 mm and 0.5 degrees off

For each, at stride 1 and 2: one evaluation against planes already on the device (wall time of the call, which clears 29 words,
launches one kernel, brings 232 bytes back and waits; and the HIP-event time of the same work on the handle's stream), and one
dsm_align_frame call (wall), split into the render (wall time of dsm_render_compose into device memory for the same sequence and
camera, depth and normal planes) and the loop (the rest of the call: iterations + 1 evaluations, each with its 232-byte download
and wait, and the solves between them), also per evaluation.  The download and the solve are NOT separated from the evaluation:
that needs events inside the entry point, and a stand-alone dsm_align_equations call costs more than an evaluation inside the loop
(it checks its arguments and orders itself behind the uploads every time), so subtracting one from the other goes negative.  p50 and min of `reps` calls after two warm-up calls.  One process on the GPU.

    python tools/bench_align.py [n_frames] [--large N] [--no-large]
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()  # before the library's first HIP call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from densesurfelmapping_amd import api, surfel_map, synth  # noqa: E402

n_frames = next((int(a) for a in sys.argv[1:] if a.isdigit() and sys.argv[sys.argv.index(a) - 1] != "--large"), 60)
n_large = int(sys.argv[sys.argv.index("--large") + 1]) if "--large" in sys.argv else 4_000_000
REPS = 10
CAMS = {"640x480": synth.VGA_DRIVE, "1226x370": synth.KITTI_1226}


def stats(times, digits=1):
    times = sorted(times)
    return {"p50": round(times[len(times) // 2], digits), "min": round(times[0], digits)}


def wall(fn, reps=REPS, warm=2):
    for _ in range(warm):
        out = fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e6)
    return times, out


def measure(ff, slot, select, segs, cam, guess):
    """ff: a FusionFunctions over the handle that holds the frame in `slot` and the map"""
    rcam = api.render_camera(cam)
    px = rcam.width * rcam.height
    d_zm = torch.empty((px,), dtype=torch.float32, device="cuda")
    d_nm = torch.empty((3 * px,), dtype=torch.float32, device="cuda")
    ptrs = {"depth": d_zm.data_ptr(), "normal": d_nm.data_ptr()}
    render_us, n_surfels = wall(lambda: ff.render(select, segs, rcam, guess, dst_ptrs=ptrs))
    out = {"surfels": n_surfels, "render_us": stats(render_us)}
    st = torch.cuda.ExternalStream(ff.stream())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for stride in (1, 2):
        prm = api.align_params(stride=stride)
        T = np.eye(4, dtype=np.float32)
        eval_us, (sums, k) = wall(lambda: ff.align_equations(slot, rcam, d_zm.data_ptr(), d_nm.data_ptr(), T, prm))
        dev = []
        for _ in range(REPS):
            ev[0].record(st)
            ff.align_equations(slot, rcam, d_zm.data_ptr(), d_nm.data_ptr(), T, prm)
            ev[1].record(st)
            ev[1].synchronize()
            dev.append(ev[0].elapsed_time(ev[1]) * 1e3)
        frame_us, res = wall(lambda: ff.align_frame(slot, select, segs, guess, model_cam=rcam, params=prm))
        e, d, f, r = stats(eval_us), stats(dev), stats(frame_us), out["render_us"]
        evals = res["iterations"] + 1
        out["stride_%d" % stride] = {
            "sampled_pixels": ((rcam.width + stride - 1) // stride) * ((rcam.height + stride - 1) // stride), "scale_log2": k,
            "pixels_at_identity": int(sums[28]), "evaluation_wall_us": e, "evaluation_device_us": d,
            "frame_wall_us": f, "status": api.ALIGN_STATUS[res["status"]], "iterations": res["iterations"], "pixels": res["n_pixels"],
            "rms_m": round(res["rms"], 5),
            "split_us_p50": {"render": r["p50"], "loop": round(f["p50"] - r["p50"], 1), "loop_per_evaluation": round((f["p50"] - r["p50"]) / evals, 1)}}
    return out


def replay(cam):
    nd = surfel_map.SurfelMap(cam, drift_free_poses=10, surfel_capacity=1 << 21)
    last = {}
    nd.set_publish(("active",), lambda pub: last.update(pub))
    for ev in synth.node_messages(cam, synth.Scene(), n_frames, lap=120):
        nd.feed(ev)
    nd.set_publish((), None)
    poses = [nd.pose(i) for i in range(nd.pose_count)]
    segs = [(q["points_begin_index"], q["n_attached"]) for q in poses if not q["is_local"] and q["n_attached"] > 0]
    guess = nd.last_pose()  # align_last's default guess
    eng = api.FusionFunctions()
    eng._h = api.C.c_void_p(nd._lib.dsm_surfel_map_engine(nd._h))
    try:
        out = {"frames": n_frames}
        out.update(measure(eng, (nd.frames_fused - 1) & 1, api.CLOUD_SELECT_MATURE, segs, cam, guess))
    finally:
        eng._h = None
    nd.close()
    return out


def large(cam, n):
    rng = np.random.default_rng(1)
    m = np.zeros(n, api.SURFEL_DTYPE)
    z = rng.uniform(1.0, 28.0, n).astype(np.float32)
    u, v = rng.uniform(0, cam.width, n), rng.uniform(0, cam.height, n)
    m["px"], m["py"], m["pz"] = (u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    m["nx"], m["ny"], m["nz"] = nrm.T
    m["size"] = rng.uniform(0.5, 3.0, n) * z / cam.fx
    m["color"] = rng.uniform(0, 255, n)
    m["weight"], m["update_times"] = 1.0, 7
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=n, frame_slots=2)
    ff.map_upload(m)
    sel = api.CLOUD_SELECT_NONZERO
    seen = ff.render(sel, (), cam, np.eye(4, dtype=np.float32), planes=("depth",))
    ff.frame_upload(0, np.zeros((cam.height, cam.width), np.uint8), seen["depth"])
    a = np.radians(0.5)
    guess = np.eye(4, dtype=np.float32)
    guess[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    guess[:3, 3] = (0.012, -0.008, 0.014)
    out = measure(ff, 0, sel, (), cam, guess)
    ff.close()
    return out


res = {"metric": "depth frame aligned to the surfel map", "reps": REPS}
for name, cam in CAMS.items():
    res[name] = {"replay": replay(cam)}
    if "--no-large" not in sys.argv:
        res[name]["large"] = large(cam, n_large)
print(json.dumps(res))
