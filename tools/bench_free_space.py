#!/usr/bin/env python
"""Cost of free space: dsm_grid_carve, dsm_grid_classify and the node's accumulator (dsm_surfel_map_set_free_space).

  carve      HIP-event time round the whole dsm_grid_carve call (the frame table's upload, the kernel, the synchronise) for 1 and 8
             frames of 1226 x 370 in the handle's slots into a set of 256 x 256 x 64 voxels of 0.1 m, DSM_CARVE_REPLACE (so that
             every call does the same work: no voxel is skipped because an earlier call freed it); warm, median and minimum
  classify   the same round dsm_grid_classify on the carved set and a map-like occupied set, all planes and the cell list
  node       frames/s through the node's callbacks at 1226 x 370 (tools/bench_node_clouds.py's stream), the accumulator off and
             on (256 x 256 x 64 voxels of 0.25 m around the first pose); alternating, the median of `rounds` each

    python tools/bench_free_space.py [--frames N] [--rounds R] [--write]
Prints one JSON line; with --write the figures, the date and the GPU's name go to profiles/free_space.md.  One process on the GPU."""
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
from densesurfelmapping_amd import api, surfel_map, synth  # noqa: E402

REPS = 25
DIMS = (256, 256, 64)


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


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


def engine_figures():
    cam = synth.KITTI_1226
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=1 << 12, frame_slots=8)
    rng = np.random.default_rng(3)
    img = np.zeros((cam.height, cam.width), np.uint8)
    for slot in range(8):  # a street-like depth: a ground plane below, walls at 6 .. 40 m, a tenth of the pixels empty
        v = np.arange(cam.height, dtype=np.float32)[:, None]
        ground = np.where(v > cam.cy + 4, 1.6 * cam.fy / np.maximum(v - cam.cy, 1.0), np.inf)
        walls = rng.uniform(6.0, 40.0, (1, cam.width)).astype(np.float32).repeat(cam.height, 0)
        dep = np.minimum(ground, walls).astype(np.float32)
        dep[rng.random(dep.shape) < 0.1] = 0.0
        ff.frame_upload(slot, img, dep)
    spec = api.grid_spec_around((0.0, 0.0, 12.0), 0.1, DIMS)
    n_words = DIMS[2] * DIMS[1] * ((DIMS[0] + 31) // 32)
    free = torch.zeros(n_words, dtype=torch.int32, device="cuda")
    poses = [np.eye(4, dtype=np.float32) for _ in range(8)]
    for k, p in enumerate(poses):
        p[:3, 3] = (0.3 * k - 1.0, 0.0, 0.5 * k)
    params = api.carve_params(near_dist=0.5, far_dist=30.0)
    out = {"dims": list(DIMS), "voxel": 0.1, "frame": [cam.width, cam.height], "reps": REPS, "carve": []}
    for n in (1, 8):
        count = [0]
        call = lambda: count.__setitem__(0, ff.grid_carve(spec, list(range(n)), poses[:n], free.data_ptr(), params, api.CARVE_REPLACE))
        p50, best = event_times(call, ff.stream())
        out["carve"].append({"frames": n, "us_p50": p50, "us_min": best, "free_voxels": count[0], "voxels": DIMS[0] * DIMS[1] * DIMS[2]})
    occ = np.zeros((DIMS[2], DIMS[1], DIMS[0]), bool)
    occ[:, DIMS[1] // 8] = True       # a floor (y is down in the camera's frame)
    occ[:, :, DIMS[0] // 5] = True    # two walls
    occ[(3 * DIMS[2]) // 4] = True
    bits = np.packbits(occ.reshape(DIMS[2], DIMS[1], DIMS[0] // 32, 4, 8), axis=-1, bitorder="little").reshape(DIMS[2], DIMS[1], DIMS[0] // 32, 4)
    occ_dev = torch.from_numpy(np.ascontiguousarray(bits).view(np.int32).reshape(-1)).cuda()
    n_vox = DIMS[0] * DIMS[1] * DIMS[2]
    planes = {"state": torch.zeros(n_vox, dtype=torch.uint8, device="cuda"), "known_free": torch.zeros(n_words, dtype=torch.int32, device="cuda"),
              "frontier": torch.zeros(n_words, dtype=torch.int32, device="cuda"), "cells": torch.zeros(n_vox, dtype=torch.int32, device="cuda")}
    ptrs = {k: t.data_ptr() for k, t in planes.items()}
    count = [0]
    call = lambda: count.__setitem__(0, ff.grid_classify(DIMS, occ_dev.data_ptr(), free.data_ptr(), ptrs, cells_cap=n_vox))
    p50, best = event_times(call, ff.stream())
    out["classify"] = {"us_p50": p50, "us_min": best, "frontier_cells": count[0]}
    ff.close()
    return out


def node_rate(events, on):
    cam = synth.KITTI_1226
    node = surfel_map.SurfelMap(cam, drift_free_poses=10, surfel_capacity=1 << 21)
    if on:
        node.set_free_space(api.grid_spec_around((0.0, 0.0, 0.0), 0.25, DIMS), dict(near_dist=0.5, far_dist=30.0, margin=0.45))
    warm = 3 * 20
    for ev in events[:warm]:
        node.feed(ev)
    node.local_surfels()
    fused0 = node.frames_fused
    t0 = time.perf_counter()
    for ev in events[warm:]:
        node.feed(ev)
    node.local_surfels()
    dt = time.perf_counter() - t0
    out = {"frames_per_s": round((node.frames_fused - fused0) / dt, 1)}
    if on:
        out["free_voxels"], out["resets"] = node.free_space()[1], node.free_space_resets
    node.close()
    return out


def main():
    n_frames, rounds = arg("--frames", 240), arg("--rounds", 3)
    res = {"metric": "free space: carve, classify, the node's accumulator", "gpu": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat()}
    res.update(engine_figures())
    events = list(synth.node_messages(synth.KITTI_1226, synth.Scene(), n_frames, lap=120))
    runs = {"off": [], "on": []}
    for _ in range(rounds):  # alternating, so that a drift of the box falls on both
        for mode in ("off", "on"):
            runs[mode].append(node_rate(events, mode == "on"))
    res["node"] = {"frames": n_frames, "rounds": rounds,
                   "off_frames_per_s": [r["frames_per_s"] for r in runs["off"]], "on_frames_per_s": [r["frames_per_s"] for r in runs["on"]],
                   "free_voxels": runs["on"][-1]["free_voxels"], "resets": runs["on"][-1]["resets"]}
    print(json.dumps(res))
    if "--write" in sys.argv:
        c1, c8 = res["carve"]
        med = lambda v: sorted(v)[len(v) // 2]
        lines = ["# Free space: one run of tools/bench_free_space.py", "",
                 "%s, %s; one process on the GPU.  HIP events round the whole call, warm, median (minimum) of %d." % (res["date"], res["gpu"], REPS), "",
                 "| what | time |", "|---|---|",
                 "| `dsm_grid_carve`, 1 frame of %d x %d into %d x %d x %d voxels (%d freed) | %.1f us (%.1f) |" % (*res["frame"], *DIMS, c1["free_voxels"], c1["us_p50"], c1["us_min"]),
                 "| `dsm_grid_carve`, 8 frames in one call (%d freed) | %.1f us (%.1f) |" % (c8["free_voxels"], c8["us_p50"], c8["us_min"]),
                 "| `dsm_grid_classify` on the result, all planes and %d frontier cells | %.1f us (%.1f) |" % (res["classify"]["frontier_cells"], res["classify"]["us_p50"], res["classify"]["us_min"]),
                 "", "The node's callbacks at %d x %d, %d frames, %d alternating rounds, frames/s:" % (*res["frame"], n_frames, rounds), "",
                 "| accumulator | rounds | median |", "|---|---|---|",
                 "| off | %s | %.1f |" % (", ".join("%.1f" % v for v in res["node"]["off_frames_per_s"]), med(res["node"]["off_frames_per_s"])),
                 "| on (%d x %d x %d voxels of 0.25 m; %d free at the end, %d resets) | %s | %.1f |"
                 % (*DIMS, res["node"]["free_voxels"], res["node"]["resets"], ", ".join("%.1f" % v for v in res["node"]["on_frames_per_s"]), med(res["node"]["on_frames_per_s"])),
                 "", "NOT measured by this tool: the carve by kernel or by counters; grids near 2^28 voxels; frame sizes other than this one; the parent",
                 "commit's node rate (the accumulator-off rows are this commit's).", "", "```json", json.dumps(res), "```", ""]
        with open(os.path.join(ROOT, "profiles", "free_space.md"), "w") as f:
            f.write("\n".join(lines))


main()
