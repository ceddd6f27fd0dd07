#!/usr/bin/env python
"""Cost of the hexagon mesh as a device product (dsm_mesh_compose, dsm_surfel_map_get_mesh / save_mesh_binary).

  engine   at 2 M and 8 M surfels, both vertex layouts: HIP-event time of dsm_mesh_compose into device memory for the map part
           (k_cloud_count + k_cloud_scan + k_mesh_scatter, every record passing) and for the store part (k_mesh_gather, one
           run over the whole store); bytes written per second and algorithmic bytes per second (map part: 44 B per record
           read twice + the vertices; store part: 44 B read + the vertices) beside the 6.0 TB/s of a plain copy (k_warp,
           profiles/r01_kernel_trace_warp_2M.md); wall time of the same call into device memory and into (pageable) host
           memory; and, on the same records, the route dsm_surfel_map_save_mesh takes today: download of the records
           (dsm_map_download for the map part, dsm_store_download for the store part), then the corner function on one host
           thread.  The two parts are measured one after the other on the same n records: first all resident in the map,
           then all deactivated into the store.
  node     one 1226x370 circuit through the node: wall time of get_mesh to host and to device, of save_mesh (ASCII) and of
           save_mesh_binary, file sizes

The host loop of today's route is tests/mesh_host.cpp (csrc/dsm_math.h's surfel_hexagon compiled for the host with g++ -O2:
the arithmetic of push_a_surfel without its std::vector push_backs), so this tool puts tests/ on sys.path and needs g++.

    python tools/bench_mesh.py [n_frames]
Prints one JSON line."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

torch.cuda.init()  # before the library's first HIP call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from densesurfelmapping_amd import api, surfel_map, synth  # noqa: E402
import mesh_cases  # noqa: E402  (the host build of the corner function)

COPY_TBPS = 6.0
n_frames = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 240


def p50(times):
    times = sorted(times)
    return times[len(times) // 2], times[0]


def engine(n, reps=10):
    rng = np.random.default_rng(1)
    m = mesh_cases.plausible_records(rng, n, api.SURFEL_DTYPE, ut=np.full(n, 7, np.int32))
    m["last_update"] = 3
    ff = api.FusionFunctions()
    ff.initialize(64, 32, 50.0, 50.0, 32.0, 16.0, 30.0, 0.3, surfel_capacity=n)
    st = torch.cuda.ExternalStream(ff.stream())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {"surfels": n}

    def device_time(select, segs, layout, dst):
        for _ in range(2):
            assert ff.mesh_compose(select, segs, layout, dst_ptr=dst.data_ptr(), cap=n) == n
        times = []
        for _ in range(reps):
            ev[0].record(st)
            ff.mesh_compose(select, segs, layout, dst_ptr=dst.data_ptr(), cap=n)
            ev[1].record(st)
            ev[1].synchronize()
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
        return p50(times)

    def device_wall(select, segs, layout, dst):
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ff.mesh_compose(select, segs, layout, dst_ptr=dst.data_ptr(), cap=n)  # (synchronises)
            times.append(time.perf_counter() - t0)
        return min(times)

    def host_time(select, segs, layout, host):
        cnt = api.C.c_int32(0)
        seg = np.asarray(segs, np.int32).reshape(-1, 2)
        b, c = np.ascontiguousarray(seg[:, 0]), np.ascontiguousarray(seg[:, 1])
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            rc = ff._lib.dsm_mesh_compose(ff._h, select, len(seg), b.ctypes.data if len(seg) else None, c.ctypes.data if len(seg) else None, layout,
                                          host.ctypes.data, 0, n, api.C.byref(cnt))
            times.append(time.perf_counter() - t0)
            assert rc == 0 and cnt.value == n
        return min(times)

    def report(us, us_min, read_bytes, layout):
        wrote = api.MESH_SURFEL_BYTES[layout] * n
        return {"us_p50": round(us, 1), "us_min": round(us_min, 1), "written_TB_per_s": round(wrote / us / 1e6, 2),
                "alg_TB_per_s": round((wrote + read_bytes) / us / 1e6, 2), "alg_frac_of_copy": round((wrote + read_bytes) / us / 1e6 / COPY_TBPS, 3)}

    ff.map_upload(m)
    for layout, name in ((api.MESH_VERTEX_REF6, "ref6"), (api.MESH_VERTEX_XYZ_RGBA8, "xyz_rgba8")):
        dst = torch.empty((n, api.MESH_SURFEL_BYTES[layout] // 4), dtype=torch.float32, device="cuda")
        us, us_min = device_time(api.CLOUD_SELECT_MATURE, (), layout, dst)
        out["map_" + name] = report(us, us_min, 2 * 44 * n, layout)
        out["map_" + name]["to_device_wall_ms"] = round(device_wall(api.CLOUD_SELECT_MATURE, (), layout, dst) * 1e3, 3)
        host = np.zeros((n, api.MESH_SURFEL_BYTES[layout] // 4), np.float32)
        out["map_" + name]["to_host_wall_ms"] = round(host_time(api.CLOUD_SELECT_MATURE, (), layout, host) * 1e3, 1)
        del dst, host
    # today's route for the map part: the records to the host, then the corner function on one thread
    def today(download, key):
        t0 = time.perf_counter()
        rec = download()
        t1 = time.perf_counter()
        verts = mesh_cases.host_vertices(rec, mesh_cases.REF6)
        t2 = time.perf_counter()
        assert len(verts) == n
        out[key] = {"download_ms": round((t1 - t0) * 1e3, 1), "host_loop_ms": round((t2 - t1) * 1e3, 1), "total_ms": round((t2 - t0) * 1e3, 1)}
        return (t2 - t0) * 1e3

    ms = min(today(ff.map_download, "today_map") for _ in range(2))
    out["today_map"]["ratio_over_get_mesh_host_ref6"] = round(ms / out["map_ref6"]["to_host_wall_ms"], 1)
    # the store part: everything deactivated into one run
    ff.store_deactivate(3)
    assert ff.store_size() == n
    for layout, name in ((api.MESH_VERTEX_REF6, "ref6"), (api.MESH_VERTEX_XYZ_RGBA8, "xyz_rgba8")):
        dst = torch.empty((n, api.MESH_SURFEL_BYTES[layout] // 4), dtype=torch.float32, device="cuda")
        us, us_min = device_time(api.CLOUD_SELECT_NONE, [(0, n)], layout, dst)
        out["store_" + name] = report(us, us_min, 44 * n, layout)
        out["store_" + name]["to_device_wall_ms"] = round(device_wall(api.CLOUD_SELECT_NONE, [(0, n)], layout, dst) * 1e3, 3)
        host = np.zeros((n, api.MESH_SURFEL_BYTES[layout] // 4), np.float32)
        out["store_" + name]["to_host_wall_ms"] = round(host_time(api.CLOUD_SELECT_NONE, [(0, n)], layout, host) * 1e3, 1)
        del dst, host
    ms = min(today(lambda: ff.store_download(0, n)[0], "today_store") for _ in range(2))
    out["today_store"]["ratio_over_get_mesh_host_ref6"] = round(ms / out["store_ref6"]["to_host_wall_ms"], 1)
    ff.close()
    return out


def node():
    cam = synth.KITTI_1226
    nd = surfel_map.SurfelMap(cam, drift_free_poses=10, surfel_capacity=1 << 21)
    for ev in synth.node_messages(cam, synth.Scene(), n_frames, lap=120):
        nd.feed(ev)
    n = int(len(nd.get_mesh(api.MESH_VERTEX_XYZ_RGBA8)))
    out = {"frames": n_frames, "surfels": n}
    for layout, name in ((api.MESH_VERTEX_REF6, "ref6"), (api.MESH_VERTEX_XYZ_RGBA8, "xyz_rgba8")):
        dst = torch.empty((n, api.MESH_SURFEL_BYTES[layout] // 4), dtype=torch.float32, device="cuda")
        th, td = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            nd.get_mesh(layout)
            t1 = time.perf_counter()
            nd.get_mesh(layout, dst_ptr=dst.data_ptr(), cap=n)
            t2 = time.perf_counter()
            th.append(t1 - t0)
            td.append(t2 - t1)
        out["get_mesh_" + name] = {"to_host_wall_ms": round(min(th) * 1e3, 3), "to_device_wall_ms": round(min(td) * 1e3, 3)}
    with tempfile.TemporaryDirectory() as d:
        for name, fn in (("save_mesh", nd.save_mesh), ("save_mesh_binary", nd.save_mesh_binary)):
            path = os.path.join(d, name + ".ply")
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn(path)
                times.append(time.perf_counter() - t0)
            out[name + "_ms"] = round(min(times) * 1e3, 1)
            out[name + "_bytes"] = os.path.getsize(path)
    out["ratio_ascii_over_binary"] = round(out["save_mesh_ms"] / out["save_mesh_binary_ms"], 1)
    nd.close()
    return out


res = {"metric": "hexagon mesh on the GPU", "copy_rate_TB_per_s": COPY_TBPS}
res["engine"] = [engine(n) for n in (2_000_000, 8_000_000)]
res["node"] = node()
print(json.dumps(res))
