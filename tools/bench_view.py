#!/usr/bin/env python
"""Cost of the viewpoint gain: dsm_grid_view and the node's dsm_surfel_map_view_gain.

  engine   HIP-event time round the whole dsm_grid_view call (the upload of the pose table, the clear, the launch, the copy of the
           scores, the synchronise), warm, median and minimum of 25, at 64 x 64 x 32 and 256 x 256 x 64 voxels with 1, 16 and 256
           poses: the map-like "surface" set of tools/bench_field.py as occupied, the free set of a node replay
           (tools/bench_free_space.py's stream and accumulator), its frontier as target; scores alone (device memory) and with the
           visible planes.  The poses are the replay's first pose (the grid lies around it) turned about its camera's y axis; the
           camera is the node's own with the carve range.  Beside each: the host checker (tests/view_host.cpp, one thread, one run) on the same inputs where it
           ends in reasonable time, the line steps it counts, and the call's two lower bounds -- the bytes of the three sets once per
           pose at the device-to-device copy rate measured here, and nothing for the steps but their number (time per step is given).
  node     wall time of dsm_surfel_map_view_gain_device (16 poses, the frontier as target) beside dsm_surfel_map_space_device on
           the same state, median of 25

    python tools/bench_view.py [--frames N] [--write]
Prints one JSON line; with --write the figures, the date and the GPU's name go to profiles/view.md.  One process on the GPU."""
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()  # before the library's first HIP call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from densesurfelmapping_amd import api, msglog, surfel_map, synth  # noqa: E402
import view_cases as vc  # noqa: E402  (the host checker)

REPS = 25
GRIDS = ((64, 64, 32), (256, 256, 64))
POSES = (1, 16, 256)
NODE_VOXEL = {(64, 64, 32): 1.0, (256, 256, 64): 0.25}  # the same 64 m x 64 m x 16 m .. 32 m around the first pose
HOST_MAX_STEPS = 2e9  # the checker is run where the smaller pose counts say it will take fewer line steps than this


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def pack(vox):
    nz, ny, nx = vox.shape
    wx = (nx + 31) // 32
    padded = np.zeros((nz, ny, wx * 32), np.uint8)
    padded[..., :nx] = vox
    bits = np.packbits(padded.reshape(nz, ny, wx, 4, 8), axis=-1, bitorder="little").reshape(nz, ny, wx, 4)
    return np.ascontiguousarray(bits).view(np.uint32).reshape(nz, ny, wx)


def surface_set(dims, rng):  # make_set("surface") of tools/bench_field.py
    nx, ny, nz = dims
    vox = np.zeros((nz, ny, nx), bool)
    vox[nz // 8] = True
    vox[:, ny // 5, : nx // 2] = True
    vox[:, :, (3 * nx) // 4] = True
    vox |= rng.random(vox.shape) < 0.002
    return pack(vox)


def event_times(call, stream, reps=REPS):
    st = torch.cuda.ExternalStream(stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(3):
        call()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        ev[0].record(st)
        call()  # (synchronises)
        ev[1].record(st)
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    times.sort()
    return round(times[len(times) // 2], 1), round(times[0], 1)


def wall_times(call, reps=REPS):
    for _ in range(3):
        call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e6)
    times.sort()
    return round(times[len(times) // 2], 1), round(times[0], 1)


def copy_rate():
    """bytes read per microsecond of a device-to-device copy of 256 MB, median of 25 (the rate a pass over the sets cannot beat)"""
    a = torch.zeros(64 << 20, dtype=torch.int32, device="cuda")
    b = torch.empty_like(a)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for k in range(REPS + 3):
        torch.cuda.synchronize()
        ev[0].record()
        b.copy_(a)
        ev[1].record()
        ev[1].synchronize()
        if k >= 3:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    times.sort()
    return a.numel() * 4 / times[len(times) // 2]


def node_state_and_figures(events, dims):
    """the free set, the frontier, the spec and the camera of the replay's final state with the pose of its first fuse (the grid lies
    around it), and the node's calls timed on that state"""
    cam = synth.KITTI_1226
    node = surfel_map.SurfelMap(cam, drift_free_poses=10, surfel_capacity=1 << 21)
    spec = api.grid_spec_around((0.0, 0.0, 0.0), NODE_VOXEL[dims], dims)
    node.set_free_space(spec, dict(near_dist=0.5, far_dist=30.0, margin=1.8 * NODE_VOXEL[dims]))
    first = None
    for ev in events:
        node.feed(ev)
        if first is None and node.frames_fused:
            first = node.last_pose()  # the grid lies around this one
    nx, ny, nz = dims
    n_vox, n_words = nx * ny * nz, nz * ny * ((nx + 31) // 32)
    frontier = torch.zeros(n_words, dtype=torch.int32, device="cuda")
    state = torch.zeros(n_vox, dtype=torch.uint8, device="cuda")
    _, n_frontier = node.space("all", dst_ptrs={"frontier": frontier.data_ptr()})
    free, n_free = node.free_space()
    q = node.view_query()
    poses = msglog.yaw_poses(first, 16)
    scores = torch.zeros(8 * len(poses), dtype=torch.int32, device="cuda")
    out = {"dims": list(dims), "voxel": NODE_VOXEL[dims], "frontier_cells": n_frontier, "free": int(n_free), "resets": node.free_space_resets, "poses": len(poses),
           "last_position": [round(float(v), 2) for v in node.last_pose()[:3, 3]]}
    out["space_us"] = wall_times(lambda: node.space("all", dst_ptrs={"state": state.data_ptr(), "frontier": frontier.data_ptr()}))
    out["view_gain_us"] = wall_times(lambda: node.view_gain(poses, "all", dst_ptrs={"scores": scores.data_ptr()}))
    got = scores.cpu().numpy().view(api.VIEW_SCORE_DTYPE)
    out["unknown_seen"] = [int(v) for v in got["unknown"]]
    bits = frontier.cpu().numpy().view(np.uint32).reshape(nz, ny, (nx + 31) // 32).copy()
    camera = vc.Cam(*(getattr(q.camera, f[0]) for f in api._RenderCamera._fields_))
    node.close()
    return {"free": free, "frontier": bits, "spec": spec, "camera": camera, "first": first}, out


def engine_figures(inputs, rate):
    ff = api.FusionFunctions.from_camera(synth.KITTI_1226, surfel_capacity=1 << 12, frame_slots=2)
    rng = np.random.default_rng(5)
    rows = []
    for dims in GRIDS:
        nx, ny, nz = dims
        inp = inputs[dims]
        occ, fre, tgt, spec, cam = surface_set(dims, rng), inp["free"], inp["frontier"], inp["spec"], inp["camera"]
        d_occ, d_fre, d_tgt = (torch.from_numpy(b.view(np.int32).reshape(-1).copy()).cuda() for b in (occ, fre, tgt))
        s = vc.make(dims, cam, origin=spec.origin[:], voxel=spec.voxel)
        set_bytes = occ.size * 4
        steps_per_pose = None
        for n in POSES:
            poses = msglog.yaw_poses(inp["first"], n)
            scores = torch.zeros(8 * n, dtype=torch.int32, device="cuda")
            visible = torch.zeros(n * occ.size, dtype=torch.int32, device="cuda")

            def call(vis):
                ff.grid_view(spec, cam, poses, d_occ.data_ptr(), d_fre.data_ptr(), d_tgt.data_ptr(), 0, None, visible.data_ptr() if vis else None, scores.data_ptr())

            only = event_times(lambda: call(False), ff.stream())
            both = event_times(lambda: call(True), ff.stream())
            got = scores.cpu().numpy().view(api.VIEW_SCORE_DTYPE)
            row = {"dims": list(dims), "poses": n, "scores_us_p50": only[0], "scores_us_min": only[1], "planes_us_p50": both[0], "planes_us_min": both[1],
                   "in_view": int(got["in_view"].sum()), "visible": int(got["visible"].sum()), "bytes_bound_us": round(3 * set_bytes * n / rate, 1)}
            if steps_per_pose is None or steps_per_pose * n <= HOST_MAX_STEPS:
                t0 = time.perf_counter()
                host = vc.host_view(s, list(poses), occ, fre, tgt)
                row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                row["steps"] = host["steps"]
                steps_per_pose = host["steps"] / n
                assert got.tobytes() == host["scores"].tobytes() and visible.cpu().numpy().view(np.uint32).tobytes() == host["visible"].tobytes()
                row["ns_per_step"] = round(only[0] * 1e3 / max(host["steps"], 1), 4)
            rows.append(row)
    ff.close()
    return rows


def main():
    n_frames = arg("--frames", 240)
    res = {"metric": "viewpoint gain: dsm_grid_view, the node's view gain", "gpu": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "reps": REPS, "frames": n_frames}
    rate = copy_rate()
    res["copy_bytes_per_us"] = round(rate, 1)
    events = list(synth.node_messages(synth.KITTI_1226, synth.Scene(), n_frames, lap=120))
    inputs, res["node"] = {}, []
    for dims in GRIDS:
        inputs[dims], figures = node_state_and_figures(events, dims)
        res["node"].append(figures)
    res["engine"] = engine_figures(inputs, rate)
    print(json.dumps(res))
    if "--write" in sys.argv:
        lines = ["# Viewpoint gain: one run of tools/bench_view.py", "",
                 "%s, %s; one process on the GPU.  HIP events round the whole `dsm_grid_view` call, warm, median (minimum) of %d: the occupied" % (res["date"], res["gpu"], REPS),
                 "set is the map-like surface set of tools/bench_field.py, the free set and the frontier (the target) are those of a node replay of %d frames," % n_frames,
                 "the poses are its first pose (the grid's centre) turned about the camera's y axis, the camera is the node's own (1226 x 370) with the carve range 0.5 .. 30 m.",
                 "The host column is tests/view_host.cpp on the same inputs, one thread, one run, and the GPU's scores and planes were compared with it byte for",
                 "byte where it ran.  Bytes bound: the three sets read once per pose at the device-to-device copy rate measured in the same process (%.0f bytes/us)." % rate, "",
                 "| grid | poses | voxels in view (visible) | scores only | scores and planes | host checker | line steps | ns per step (scores only) | bytes bound |",
                 "|---|---|---|---|---|---|---|---|---|"]
        for r in res["engine"]:
            host = ("%.1f ms" % r["host_ms"], "%d" % r["steps"], "%.4f" % r["ns_per_step"]) if "host_ms" in r else ("not run", "not counted", "-")
            lines.append("| %d x %d x %d | %d | %d (%d) | %.1f us (%.1f) | %.1f us (%.1f) | %s | %s | %s | %.1f us |"
                         % (*r["dims"], r["poses"], r["in_view"], r["visible"], r["scores_us_p50"], r["scores_us_min"], r["planes_us_p50"], r["planes_us_min"], *host, r["bytes_bound_us"]))
        lines += ["", "The node after the same replay, wall time of the whole call, device destinations, 16 poses, median (minimum) of %d:" % REPS, "",
                  "| grid (voxel) | free voxels | frontier cells | `space_device` (state, frontier) | `view_gain_device` (scores, frontier target) |", "|---|---|---|---|---|"]
        for r in res["node"]:
            lines.append("| %d x %d x %d (%.2f m) | %d | %d | %.1f us (%.1f) | %.1f us (%.1f) |" % (*r["dims"], r["voxel"], r["free"], r["frontier_cells"], *r["space_us"], *r["view_gain_us"]))
        lines += ["", "How far from the bounds: see the two right-hand columns -- the measured time over the bytes bound says how little of the call is the pass over",
                  "the sets (the line walks are the work); the time per line step is an upper estimate of what a step costs, since the kernel stops a walk at its",
                  "first blocker and where the line leaves the grid, while the checker counts every interior point of every voxel in view.", "",
                  "NOT measured by this tool: hardware counters; the split of a call between the launch, the pose upload and the copy of the scores (no trace was",
                  "taken); the checker at the pose counts marked 'not run'; DSM_VIEW_UNKNOWN_BLOCKS; cameras far outside the grid; grids near 2^28 voxels; a variant",
                  "staging tiles of the sets in LDS (none was written).", "", "```json", json.dumps(res), "```", ""]
        with open(os.path.join(ROOT, "profiles", "view.md"), "w") as f:
            f.write("\n".join(lines))


main()
