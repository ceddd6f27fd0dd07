#!/usr/bin/env python
"""Cost of the surfel map as an occupancy voxel grid (dsm_grid_compose, dsm_grid_inflate), beside the host path it replaces.

  replay   the map a node grows over a 1226x370 circuit (n_frames frames), kind ALL, in a grid around the final fuse pose
  large    a 3 M-surfel map made on the host (surfels spread through the volume of the 0.2 m grid), select NONZERO

For each, at 0.1 m and 0.2 m voxels in a 256 x 256 x 64 grid: HIP-event time of a compose into device memory without the index
plane (occupied + cells: the bits are splatted directly) and with it (index + occupied + cells: atomicMin, then the bits pass),
p50 and min of `reps` calls after two warm-up calls, the wall time of the same into host memory, the share of voxels occupied --
and of dsm_grid_inflate alone on the occupied set at r = 0, 3 and 8.  The host path: every surfel record to the host
(map_download + store_download / the node's taps) and a numpy voxelisation of the CENTRES (floor, unique) -- less than the grid
computes (no disc extent, no inflation), so the comparison flatters the host.  One process on the GPU.

    python tools/bench_grid.py [n_frames] [--no-large]
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

n_frames = next((int(a) for a in sys.argv[1:] if a.isdigit()), 120)
CAM = synth.KITTI_1226
REPS = 10
DIMS = (256, 256, 64)
VOXELS = (0.1, 0.2)
RADII = (0, 3, 8)


def p50(times):
    times = sorted(times)
    return round(times[len(times) // 2], 1), round(times[0], 1)


def event_time(call, stream):
    st = torch.cuda.ExternalStream(stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(2):
        call()
    times = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        ev[0].record(st)
        call()  # (synchronises)
        ev[1].record(st)
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return p50(times)


def wall(fn, reps=2):
    best, out = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t = (time.perf_counter() - t0) * 1e3
        best = t if best is None else min(best, t)
    return round(best, 2), out


def host_voxelise(records, spec):
    """the centres' voxels: the least a host voxelisation does"""
    p = np.stack([records["px"], records["py"], records["pz"]], 1)
    p = p[np.isfinite(p).all(1)]
    f = np.floor((p - np.array(spec.origin[:], np.float32)) / np.float32(spec.voxel))
    ijk = f[((f >= 0) & (f < np.array([spec.nx, spec.ny, spec.nz], np.float32))).all(1)].astype(np.int64)
    return np.unique((ijk[:, 2] * spec.ny + ijk[:, 1]) * spec.nx + ijk[:, 0])


def measure(compose, inflate, download, centre, stream):
    """compose(spec, planes, dst_ptrs, cells_cap) / inflate(dims, r, src, dst) / download() -> records"""
    out = {}
    for voxel in VOXELS:
        spec = api.grid_spec_around(centre, voxel, DIMS, 0)
        wx, bits_shape, index_shape = api.grid_shapes(spec)
        n_words, n_vox = int(np.prod(bits_shape)), int(np.prod(index_shape))
        bufs = {"occupied": torch.zeros(n_words, dtype=torch.int32, device="cuda"), "inflated": torch.zeros(n_words, dtype=torch.int32, device="cuda"),
                "index": torch.zeros(n_vox, dtype=torch.int32, device="cuda"), "cells": torch.zeros(n_vox, dtype=torch.int32, device="cuda")}
        ptr = lambda *ks: {k: bufs[k].data_ptr() for k in ks}
        r = {}
        n, cells = compose(spec, None, ptr("occupied", "cells"), n_vox)
        r["surfels"], r["cells"], r["occupied_share"] = n, cells, round(cells / n_vox, 4)
        r["compose_bits_us_p50"], r["compose_bits_us_min"] = event_time(lambda: compose(spec, None, ptr("occupied", "cells"), n_vox), stream)
        r["compose_index_us_p50"], r["compose_index_us_min"] = event_time(lambda: compose(spec, None, ptr("index", "occupied", "cells"), n_vox), stream)
        r["compose_to_host_wall_ms"], _ = wall(lambda: compose(spec, ("occupied", "cells"), None, None))
        for rad in RADII:
            us, us_min = event_time(lambda: inflate(DIMS, rad, bufs["occupied"].data_ptr(), bufs["inflated"].data_ptr()), stream)
            r["inflate_r%d_us_p50" % rad], r["inflate_r%d_us_min" % rad] = us, us_min
        ms, rec = wall(download)
        r["host_download_wall_ms"], r["host_download_bytes"] = ms, int(rec.nbytes)
        ms, host_cells = wall(lambda: host_voxelise(rec, spec))
        r["host_numpy_voxelise_wall_ms"], r["host_centre_cells"] = ms, int(len(host_cells))
        out["voxel_%g" % voxel] = r
    return out


def replay():
    nd = surfel_map.SurfelMap(CAM, drift_free_poses=10, surfel_capacity=1 << 21)
    for ev in synth.node_messages(CAM, synth.Scene(), n_frames, lap=120):
        nd.feed(ev)
    eng = api.C.c_void_p(nd._lib.dsm_surfel_map_engine(nd._h))
    stream = api.C.c_void_p()
    nd._lib.dsm_stream.argtypes = [api.C.c_void_p, api.C.POINTER(api.C.c_void_p)]
    assert nd._lib.dsm_stream(eng, api.C.byref(stream)) == 0
    api.load_library()  # (the argument types of dsm_grid_inflate)

    def compose(spec, planes, dst_ptrs, cells_cap):
        if dst_ptrs is not None:
            return nd.grid("all", spec=spec, dst_ptrs=dst_ptrs, cells_cap=cells_cap)
        return nd.grid("all", spec=spec, planes=planes)

    def inflate(dims, r, src, dst):
        assert nd._lib.dsm_grid_inflate(eng, dims[0], dims[1], dims[2], r, api.C.c_void_p(src), api.C.c_void_p(dst)) == 0

    def download():
        return np.concatenate([nd.attached_surfels(i) for i in range(nd.pose_count)] + [nd.local_surfels()])

    out = {"frames": n_frames}
    out.update(measure(compose, inflate, download, nd.last_pose()[:3, 3], stream.value))
    nd.close()
    return out


def large(n=3_000_000):
    rng = np.random.default_rng(1)
    m = np.zeros(n, api.SURFEL_DTYPE)
    half = np.array(DIMS) * max(VOXELS) / 2
    p = rng.uniform(-half, half, (n, 3))
    m["px"], m["py"], m["pz"] = p.T
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    m["nx"], m["ny"], m["nz"] = nrm.T
    m["size"] = rng.uniform(0.02, 0.15, n)
    m["weight"], m["update_times"] = 1.0, 7
    ff = api.FusionFunctions.from_camera(CAM, surfel_capacity=n)
    ff.map_upload(m)
    sel = api.CLOUD_SELECT_NONZERO

    def compose(spec, planes, dst_ptrs, cells_cap):
        if dst_ptrs is not None:
            return ff.grid(sel, (), spec, dst_ptrs=dst_ptrs, cells_cap=cells_cap)
        return ff.grid(sel, (), spec, planes=planes)

    out = measure(compose, ff.grid_inflate, ff.map_download, (0.0, 0.0, 0.0), ff.stream())
    ff.close()
    return out


res = {"metric": "surfel map as a voxel grid", "dims": list(DIMS), "reps": REPS}
res["replay"] = replay()
if "--no-large" not in sys.argv:
    res["large"] = large()
print(json.dumps(res))
