#!/usr/bin/env python
"""Cost of the node's point-cloud topics (dsm_surfel_map_set_publish / dsm_cloud_compose / dsm_frame_cloud).

  node       frames/s through the node's callbacks at 1226x370 (tools/bench_node.py's stream): publication off, the
             reference's default set {ACTIVE, INACTIVE}, all five kinds -- and the same two clouds the only way there was
             before (full dsm_map_download + dsm_store_download after every fuse, filtered on the host)
  compaction HIP-event time of dsm_cloud_compose(MATURE) into device memory over random maps of 250 k, 2 M and 8 M records;
             algorithmic bytes = 44 B per record (count pass) + 44 B per record (scatter pass) + 16 B per written point,
             as a fraction of 8 TB/s

    python tools/bench_node_clouds.py [n_frames]
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()  # before the library's first HIP call
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densesurfelmapping_amd import api, surfel_map, synth  # noqa: E402

n_frames = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 240
cam = synth.KITTI_1226
events = list(synth.node_messages(cam, synth.Scene(), n_frames, lap=120))


def node_rate(mode):
    node = surfel_map.SurfelMap(cam, drift_free_poses=10, surfel_capacity=1 << 21)
    points = [0]
    if mode in ("default", "all"):
        kinds = ("active", "inactive") if mode == "default" else surfel_map.CLOUD_KINDS
        node.set_publish(kinds, lambda pub: points.__setitem__(0, points[0] + sum(len(c) for c in pub["clouds"].values())))
    warm = 3 * 20
    for ev in events[:warm]:
        node.feed(ev)
    node.local_surfels()
    fused0 = node.frames_fused
    t0 = time.perf_counter()
    for ev in events[warm:]:
        node.feed(ev)
        if mode == "download" and ev[0] == "orb":  # what a caller had to do per frame before
            local = node.local_surfels()
            local = local[local["update_times"] >= 5]
            active = np.stack([local["px"], local["py"], local["pz"], local["color"]], axis=1)
            inactive = node.inactive_cloud()
            points[0] += len(active) + len(inactive)
    node.local_surfels()
    dt = time.perf_counter() - t0
    out = {"frames_per_s": round((node.frames_fused - fused0) / dt, 1), "points_per_frame": round(points[0] / max(node.frames_fused - fused0, 1)),
           "local_surfels": len(node.local_surfels()), "inactive_points": len(node.inactive_cloud())}
    node.close()
    return out


def compaction(n, reps=20):
    import torch
    rng = np.random.default_rng(1)
    ff = api.FusionFunctions()
    ff.initialize(64, 32, 50.0, 50.0, 32.0, 16.0, 30.0, 0.3, surfel_capacity=n)
    m = np.zeros(n, api.SURFEL_DTYPE)
    m["px"] = rng.random(n, dtype=np.float32)
    m["update_times"] = rng.integers(0, 10, n)  # half of the records pass update_times >= 5
    ff.map_upload(m)
    dst = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    st = torch.cuda.ExternalStream(ff.stream())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    k = 0
    for _ in range(3):
        k = ff.cloud_compose(api.CLOUD_SELECT_MATURE, dst_ptr=dst.data_ptr(), cap=n)
    times = []
    for _ in range(reps):
        ev[0].record(st)
        ff.cloud_compose(api.CLOUD_SELECT_MATURE, dst_ptr=dst.data_ptr(), cap=n)
        ev[1].record(st)
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    times.sort()
    us = times[len(times) // 2]
    alg = 44 * n * 2 + 16 * k
    ff.close()
    return {"records": n, "points": k, "us_p50": round(us, 1), "us_min": round(times[0], 1), "alg_bytes": alg,
            "TB_per_s": round(alg / us / 1e6, 2), "frac_of_8TBps": round(alg / us / 1e6 / 8.0, 3)}


res = {"metric": "point-cloud publication cost", "workload": "1226x370 circuit of 120 frames (bench_node.py), drift_free_poses 10"}
for mode in ("off", "default", "all", "download"):
    res["node_" + mode] = node_rate(mode)
res["compaction"] = [compaction(n) for n in (250_000, 2_000_000, 8_000_000)]
print(json.dumps(res))
