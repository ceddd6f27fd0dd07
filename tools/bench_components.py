#!/usr/bin/env python
"""Cost of connected components: dsm_grid_components and the node's dsm_surfel_map_frontier_clusters.

  engine   HIP-event time round the whole dsm_grid_components call (its launches, the read-back of the two counts, the synchronise),
           warm, median and minimum of 25, on three sets -- the map-like "surface" set of tools/bench_field.py, the frontier of a node
           replay (tools/bench_free_space.py's stream and accumulator), a random set at density 0.31 -- at 64 x 64 x 32 and
           256 x 256 x 64 voxels, with 6 and 26, with the label plane alone and with the table (min_count 1); beside each the time of
           the host checker (tests/components_host.cpp, one thread, flood fill) on the same set
  node     wall time of dsm_surfel_map_frontier_clusters_device (with and without reachability) beside dsm_surfel_map_space_device
           on the same state, median of 25

    python tools/bench_components.py [--frames N] [--write]
Prints one JSON line; with --write the figures, the date and the GPU's name go to profiles/components.md.  One process on the GPU."""
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
from densesurfelmapping_amd import api, surfel_map, synth  # noqa: E402
import components_cases as cc  # noqa: E402  (the host checker)

REPS = 25
GRIDS = ((64, 64, 32), (256, 256, 64))
NODE_VOXEL = {(64, 64, 32): 1.0, (256, 256, 64): 0.25}  # the same 64 m x 64 m x 16 m .. 32 m around the first pose


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


def node_state_and_figures(events, dims):
    """the frontier words of the replay's final state, and the node's calls timed on it"""
    cam = synth.KITTI_1226
    node = surfel_map.SurfelMap(cam, drift_free_poses=10, surfel_capacity=1 << 21)
    spec = api.grid_spec_around((0.0, 0.0, 0.0), NODE_VOXEL[dims], dims)
    node.set_free_space(spec, dict(near_dist=0.5, far_dist=30.0, margin=1.8 * NODE_VOXEL[dims]))
    for ev in events:
        node.feed(ev)
    nx, ny, nz = dims
    n_vox, n_words = nx * ny * nz, nz * ny * ((nx + 31) // 32)
    frontier = torch.zeros(n_words, dtype=torch.int32, device="cuda")
    state = torch.zeros(n_vox, dtype=torch.uint8, device="cuda")
    _, n_frontier = node.space("all", dst_ptrs={"frontier": frontier.data_ptr()})
    origin = node.last_pose()[:3, 3]
    label = torch.zeros(n_vox, dtype=torch.int32, device="cuda")
    table = torch.zeros(8 * max(n_frontier, 1), dtype=torch.int64, device="cuda")
    ptrs = {"table": table.data_ptr(), "label": label.data_ptr()}
    out = {"dims": list(dims), "voxel": NODE_VOXEL[dims], "frontier_cells": n_frontier, "resets": node.free_space_resets}
    out["space_us"] = wall_times(lambda: node.space("all", dst_ptrs={"state": state.data_ptr(), "frontier": frontier.data_ptr()}))
    res = [None]
    out["clusters_us"] = wall_times(lambda: res.__setitem__(0, node.frontier_clusters("all", 26, 1, dst_ptrs=ptrs, table_cap=max(n_frontier, 1))))
    out["clusters"], out["clusters_all"] = res[0][0], res[0][1]
    out["clusters_from_us"] = wall_times(lambda: res.__setitem__(0, node.frontier_clusters("all", 26, 1, origin=origin, dst_ptrs=ptrs, table_cap=max(n_frontier, 1))))
    out["from_root"] = res[0][2]
    t = table.cpu().numpy().view(api.COMPONENT_DTYPE)[: out["clusters"]]
    out["reachable"] = int((t["tag"] == out["from_root"]).sum()) if out["from_root"] >= 0 else 0
    bits = frontier.cpu().numpy().view(np.uint32).reshape(nz, ny, (nx + 31) // 32).copy()
    node.close()
    return bits, out


def engine_figures(sets):
    ff = api.FusionFunctions.from_camera(synth.KITTI_1226, surfel_capacity=1 << 12, frame_slots=2)
    rows = []
    for dims in GRIDS:
        nx, ny, nz = dims
        n_vox = nx * ny * nz
        label = torch.zeros(n_vox, dtype=torch.int32, device="cuda")
        for name, bits in sets[dims].items():
            src = torch.from_numpy(bits.view(np.int32).reshape(-1)).cuda()
            for conn in (6, 26):
                t0 = time.perf_counter()
                host = cc.host_components(bits, nx, conn)
                host_ms = (time.perf_counter() - t0) * 1e3
                cap = max(host["n"], 1)
                table = torch.zeros(8 * cap, dtype=torch.int64, device="cuda")
                res = [None]
                only = event_times(lambda: res.__setitem__(0, ff.grid_components(dims, src.data_ptr(), conn, 1, label_ptr=label.data_ptr())), ff.stream())
                assert res[0] == (host["n"], host["n_all"]) and np.array_equal(label.cpu().numpy().reshape(nz, ny, nx), host["label"])
                both = event_times(lambda: res.__setitem__(0, ff.grid_components(dims, src.data_ptr(), conn, 1, label_ptr=label.data_ptr(),
                                                                                 table_ptr=table.data_ptr(), table_cap=cap)), ff.stream())
                assert table.cpu().numpy().view(api.COMPONENT_DTYPE)[: host["n"]].tobytes() == host["table"].tobytes()
                rows.append({"dims": list(dims), "set": name, "density": round(float(np.unpackbits(bits.view(np.uint8)).mean()), 4), "connectivity": conn,
                             "components": host["n_all"], "largest": int(host["table"]["count"].max()) if host["n"] else 0,
                             "label_us_p50": only[0], "label_us_min": only[1], "table_us_p50": both[0], "table_us_min": both[1], "host_ms": round(host_ms, 1)})
    ff.close()
    return rows


def main():
    n_frames = arg("--frames", 240)
    res = {"metric": "connected components: dsm_grid_components, the node's frontier clusters", "gpu": torch.cuda.get_device_name(0),
           "date": datetime.date.today().isoformat(), "reps": REPS, "frames": n_frames}
    events = list(synth.node_messages(synth.KITTI_1226, synth.Scene(), n_frames, lap=120))
    rng = np.random.default_rng(5)
    sets, res["node"] = {}, []
    for dims in GRIDS:
        frontier, figures = node_state_and_figures(events, dims)
        res["node"].append(figures)
        sets[dims] = {"surface": surface_set(dims, rng), "frontier": frontier, "random 0.31": pack(rng.random(dims[::-1]) < 0.31)}
    res["engine"] = engine_figures(sets)
    print(json.dumps(res))
    if "--write" in sys.argv:
        lines = ["# Connected components: one run of tools/bench_components.py", "",
                 "%s, %s; one process on the GPU.  HIP events round the whole `dsm_grid_components` call, warm, median (minimum) of %d;" % (res["date"], res["gpu"], REPS),
                 "the host column is tests/components_host.cpp's flood fill on the same set, one thread, one run.", "",
                 "| grid | set (density) | connectivity | components (largest) | label only | label and table | host checker |", "|---|---|---|---|---|---|---|"]
        for r in res["engine"]:
            lines.append("| %d x %d x %d | %s (%.4f) | %d | %d (%d) | %.1f us (%.1f) | %.1f us (%.1f) | %.1f ms |"
                         % (*r["dims"], r["set"], r["density"], r["connectivity"], r["components"], r["largest"], r["label_us_p50"], r["label_us_min"],
                            r["table_us_p50"], r["table_us_min"], r["host_ms"]))
        lines += ["", "The node after %d frames of 1226 x 370 (tools/bench_free_space.py's stream), wall time of the whole call, device destinations," % n_frames,
                  "median (minimum) of %d:" % REPS, "",
                  "| grid (voxel) | frontier cells | clusters | `space_device` (state, frontier) | `frontier_clusters_device` | ... with `from` (reachable) |", "|---|---|---|---|---|---|"]
        for r in res["node"]:
            lines.append("| %d x %d x %d (%.2f m) | %d | %d | %.1f us (%.1f) | %.1f us (%.1f) | %.1f us (%.1f) (%d of %d) |"
                         % (*r["dims"], r["voxel"], r["frontier_cells"], r["clusters"], *r["space_us"], *r["clusters_us"], *r["clusters_from_us"], r["reachable"], r["clusters"]))
        lines += ["", "NOT measured by this tool: hardware counters; the split of a call by kernel (no trace was taken); grids near 2^26 voxels; sets built to",
                  "make the union-find's chains long (a serpentine through a large grid); min_count above 1.", "", "```json", json.dumps(res), "```", ""]
        with open(os.path.join(ROOT, "profiles", "components.md"), "w") as f:
            f.write("\n".join(lines))


main()
