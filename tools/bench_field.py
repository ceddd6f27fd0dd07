#!/usr/bin/env python
"""Cost of the truncated Euclidean distance field (dsm_grid_distance) on a bit set resident in device memory, beside
dsm_grid_inflate at radius 16 on the same set: the one comparable kernel in the tree.

Grids 256 x 256 x 64 and 64 x 64 x 32, max_dist 4, 16 and 64, all three planes written.  The walks of the y and z passes stop
early where an obstacle is near and are skipped where a tile column is empty, so the time depends on the set; three are timed:
  surface  a floor, two walls and scattered voxels, about 3 % set: what a map looks like
  empty    nothing set: no lane walks
  dense    half the voxels set at random: every walk stops at once
HIP-event time round the whole call (the table upload, the three kernels, the synchronise), warm (three calls first), median and
minimum of `reps` calls.  Bytes: what the three passes must move per voxel -- the bits (1/8), the byte plane written and read
(1 + 1), the word plane written and read (4 + 4), the planes written (2 + 4 + 4) = 20.1 -- and the same with every tile's halo
re-read counted ((64 + 2 max_dist) / 64 of the two reads); bytes per second is the first over the median.  One process on the GPU.

    python tools/bench_field.py [--case NX NY NZ MAX_DIST SET [REPS]]
Prints one JSON line.  --case runs one configuration alone (for a kernel trace of its own)."""
import json
import os
import sys

import numpy as np
import torch

torch.cuda.init()  # before the library's first HIP call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from densesurfelmapping_amd import api, synth  # noqa: E402

REPS = 25
GRIDS = ((256, 256, 64), (64, 64, 32))
MAX_DISTS = (4, 16, 64)
SETS = ("surface", "empty", "dense")
VOXEL = 0.1
INFLATE_RADIUS = 16


def make_set(name, dims, rng):
    nx, ny, nz = dims
    vox = np.zeros((nz, ny, nx), bool)
    if name == "surface":
        vox[nz // 8] = True                  # a floor
        vox[:, ny // 5, : nx // 2] = True    # two walls
        vox[:, :, (3 * nx) // 4] = True
        vox |= rng.random(vox.shape) < 0.002
    elif name == "dense":
        vox = rng.random(vox.shape) < 0.5
    wx = (nx + 31) // 32
    padded = np.zeros((nz, ny, wx * 32), np.uint8)
    padded[..., :nx] = vox
    bits = np.packbits(padded.reshape(nz, ny, wx, 4, 8), axis=-1, bitorder="little").reshape(nz, ny, wx, 4)
    return np.ascontiguousarray(bits).view(np.uint32).reshape(nz, ny, wx), float(vox.mean())


def event_times(call, stream, reps):
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


def field_bytes(n_vox, max_dist):
    """(the least the three passes move, the same with the halo re-reads) in bytes"""
    halo = (64 + 2 * max_dist) / 64
    return n_vox * (1 / 8 + 1 + 1 + 4 + 4 + 10), n_vox * (1 / 8 + 1 + halo + 4 + 4 * halo + 10)


def run_case(ff, dims, max_dist, name, reps):
    nx, ny, nz = dims
    n_vox = nx * ny * nz
    bits, share = make_set(name, dims, np.random.default_rng(7))
    src = torch.from_numpy(bits.view(np.int32)).cuda()
    planes = {"dist2": torch.zeros(n_vox, dtype=torch.int16, device="cuda"), "nearest": torch.zeros(n_vox, dtype=torch.int32, device="cuda"),
              "distance": torch.zeros(n_vox, dtype=torch.float32, device="cuda")}
    ptrs = {k: t.data_ptr() for k, t in planes.items()}
    p50, best = event_times(lambda: ff.grid_distance(dims, max_dist, VOXEL, src.data_ptr(), ptrs), ff.stream(), reps)
    least, with_halo = field_bytes(n_vox, max_dist)
    found = int((planes["nearest"] >= 0).sum().item())
    return {"dims": list(dims), "max_dist": max_dist, "set": name, "set_share": round(share, 4), "reached_share": round(found / n_vox, 4),
            "field_us_p50": p50, "field_us_min": best, "bytes_least": int(least), "bytes_with_halo": int(with_halo),
            "gbytes_per_s_least": round(least / (p50 * 1e-6) / 1e9, 1)}


def run_inflate(ff, dims, name, reps):
    nx, ny, nz = dims
    bits, _ = make_set(name, dims, np.random.default_rng(7))
    src = torch.from_numpy(bits.view(np.int32)).cuda()
    dst = torch.zeros_like(src)
    p50, best = event_times(lambda: ff.grid_inflate(dims, INFLATE_RADIUS, src.data_ptr(), dst.data_ptr()), ff.stream(), reps)
    return {"dims": list(dims), "radius": INFLATE_RADIUS, "set": name, "inflate_us_p50": p50, "inflate_us_min": best}


ff = api.FusionFunctions.from_camera(synth.KITTI_1226, surfel_capacity=1 << 12)
res = {"metric": "distance field of a resident bit set", "voxel": VOXEL}
if "--case" in sys.argv:
    a = sys.argv[sys.argv.index("--case") + 1:]
    reps = int(a[5]) if len(a) > 5 else REPS
    res["reps"] = reps
    res["field"] = [run_case(ff, (int(a[0]), int(a[1]), int(a[2])), int(a[3]), a[4], reps)]
else:
    res["reps"] = REPS
    res["field"] = [run_case(ff, g, r, s, REPS) for g in GRIDS for s in SETS for r in MAX_DISTS]
    res["inflate"] = [run_inflate(ff, g, s, REPS) for g in GRIDS for s in SETS]
ff.close()
print(json.dumps(res))
