#!/usr/bin/env python
"""Cost of rendering the surfel map to images (dsm_render_compose) at 1226x370, beside today's alternative.

  replay   the map a node grows over a 1226x370 circuit (n_frames frames; 240 give about 390 k surfels), rendered as kind ALL
           from the final fuse pose with the node's camera
  large    an 8 M-surfel map made on the host (surfels spread through the camera's view volume, as tools/map_kernels_8m.py makes
           a map for the map-sized kernels), rendered with select NONZERO

For each: HIP-event time of the whole call into device memory (all four planes; clear + set-up + both splat tiers + resolve
and the small uploads in front, p50 and min of `reps` calls after two warm-up calls), wall time of the same call into device
and into host memory, the share of pixels covered -- and what a caller does today to get an image: all vertices (get_mesh /
mesh_compose) or all points (get_cloud / cloud_compose) to the host, wall time and bytes, before any host rasteriser has run.
The split by kernel is not taken here (the call is one entry point): run this tool under `rocprofv3 --kernel-trace --stats -- python
tools/bench_render.py` for it.  One process on the GPU.

    python tools/bench_render.py [n_frames] [--no-large]
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

n_frames = next((int(a) for a in sys.argv[1:] if a.isdigit()), 240)
CAM = synth.KITTI_1226
REPS = 10


def p50(times):
    times = sorted(times)
    return round(times[len(times) // 2], 1), round(times[0], 1)


def measure(render_device, render_host, stream):
    """render_device(ptrs) / render_host() -> planes dict; returns the figures of one configuration"""
    rcam = api.render_camera(CAM)
    bufs = {k: torch.empty((rcam.height * rcam.width * (3 if k == "normal" else 1),),
                           dtype={"depth": torch.float32, "index": torch.int32, "normal": torch.float32, "intensity": torch.uint8}[k], device="cuda")
            for k in api.RENDER_PLANES}
    ptrs = {k: t.data_ptr() for k, t in bufs.items()}
    st = torch.cuda.ExternalStream(stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(2):
        n = render_device(ptrs)
    times, walls = [], []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record(st)
        render_device(ptrs)  # (synchronises)
        ev[1].record(st)
        ev[1].synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    host_walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        planes = render_host()
        host_walls.append((time.perf_counter() - t0) * 1e3)
    us, us_min = p50(times)
    return {"surfels": n, "device_us_p50": us, "device_us_min": us_min, "to_device_wall_ms": round(min(walls), 3),
            "to_host_wall_ms": round(min(host_walls), 3), "covered": round(float((planes["index"] >= 0).mean()), 3),
            "ns_per_surfel": round(us * 1e3 / max(n, 1), 2)}


def timed(fn):
    best, out = None, None
    for _ in range(2):
        t0 = time.perf_counter()
        out = fn()
        t = (time.perf_counter() - t0) * 1e3
        best = t if best is None else min(best, t)
    return round(best, 1), out


def replay():
    nd = surfel_map.SurfelMap(CAM, drift_free_poses=10, surfel_capacity=1 << 21)
    for ev in synth.node_messages(CAM, synth.Scene(), n_frames, lap=120):
        nd.feed(ev)
    eng = api.C.c_void_p(nd._lib.dsm_surfel_map_engine(nd._h))
    stream = api.C.c_void_p()
    nd._lib.dsm_stream.argtypes = [api.C.c_void_p, api.C.POINTER(api.C.c_void_p)]
    assert nd._lib.dsm_stream(eng, api.C.byref(stream)) == 0
    out = {"frames": n_frames}
    out.update(measure(lambda ptrs: nd.render("all", dst_ptrs=ptrs), lambda: nd.render("all"), stream.value))
    ms, mesh = timed(lambda: nd.get_mesh(api.MESH_VERTEX_XYZ_RGBA8))
    out["today_get_mesh"] = {"to_host_wall_ms": ms, "bytes": int(mesh.nbytes)}
    ms, cloud = timed(lambda: nd.cloud("all"))
    out["today_get_cloud"] = {"to_host_wall_ms": ms, "bytes": int(cloud.nbytes)}
    nd.close()
    return out


def large(n=8_000_000):
    rng = np.random.default_rng(1)
    m = np.zeros(n, api.SURFEL_DTYPE)
    z = rng.uniform(1.0, 28.0, n).astype(np.float32)
    u, v = rng.uniform(0, CAM.width, n), rng.uniform(0, CAM.height, n)
    m["px"], m["py"], m["pz"] = (u - CAM.cx) / CAM.fx * z, (v - CAM.cy) / CAM.fy * z, z
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    m["nx"], m["ny"], m["nz"] = nrm.T
    m["size"] = rng.uniform(0.5, 3.0, n) * z / CAM.fx  # discs of one to six pixels across, face on
    m["color"] = rng.uniform(0, 255, n)
    m["weight"], m["update_times"] = 1.0, 7
    ff = api.FusionFunctions.from_camera(CAM, surfel_capacity=n)
    ff.map_upload(m)
    pose = np.eye(4, dtype=np.float32)
    sel = api.CLOUD_SELECT_NONZERO
    out = measure(lambda ptrs: ff.render(sel, (), CAM, pose, dst_ptrs=ptrs), lambda: ff.render(sel, (), CAM, pose), ff.stream())
    ms, mesh = timed(lambda: ff.mesh_compose(sel, (), api.MESH_VERTEX_XYZ_RGBA8))
    out["today_mesh_compose"] = {"to_host_wall_ms": ms, "bytes": int(mesh.nbytes)}
    ms, cloud = timed(lambda: ff.cloud_compose(sel, ()))
    out["today_cloud_compose"] = {"to_host_wall_ms": ms, "bytes": int(cloud.nbytes)}
    ff.close()
    return out


res = {"metric": "surfel map rendered to images", "image": [CAM.width, CAM.height], "reps": REPS}
res["replay"] = replay()
if "--no-large" not in sys.argv:
    res["large"] = large()
print(json.dumps(res))
