"""Recorded message streams for the node (the ROS-free replay driver of SURVEY.md §8(f) rank 3).

A log holds, in publication order, exactly what the node's three subscribers would receive
(ros_node.cpp:24-32): mono8 images, 32FC1 depth images and the synchronised ORB-SLAM triple
(loop_stamps, loop_path, this_pose).  Little-endian binary, one header, then records:

    header : int32 width, height, drift_free_poses;  float32 fx, fy, cx, cy, far, near
    record : int32 kind (0 image, 1 depth, 2 orb, -1 end of log), uint32 sec, uint32 nsec, payload
       image : width*height uint8          depth : width*height float32
       orb   : int32 n_values, float32 values[n_values]      (channels[0].values: pairs of keyframe indices)
               int32 n_path,   float64 path[n_path][7]       (px py pz qx qy qz qw)
               float64 pose[7], float64 covariance[36]       ([0] > 0: new keyframe, [1]: reference keyframe)

tests/cpp/node_replay_test.cpp reads the same format through include/dsm_surfel_map.hpp.

    python -m densesurfelmapping_amd.msglog LOG --save-cloud map.PCD --save-mesh map_mesh.PLY

--save-grid PATH.npz writes the whole map as an occupancy voxel grid around the final fuse pose (--grid-voxel V, --grid-dims NX NY NZ,
--grid-inflate R): origin, voxel, dims, inflate, the occupied and inflated bit sets and the occupied cells.

--save-field PATH.npz writes the truncated Euclidean distance field of that grid's occupied set out to --field-max-dist R voxels
(same --grid-voxel and --grid-dims): origin, voxel, dims, max_dist, dist2, nearest, distance.

--save-space PATH.npz switches the node's free-space accumulator on before the replay, in a grid of --grid-dims voxels of --grid-voxel
metres around the FIRST pose of the log (--carve-near N, --carve-far F, --carve-margin M: the carve's range and clearance), and writes
origin, voxel, dims, near, far, margin, state [nz][ny][nx] (0 unknown, 1 free, 2 occupied), frontier_cells, free, n_free and resets
(how often a loop closure cleared the set: after one it holds only the frames fused since).

--save-frontier-clusters PATH.npz uses the same accumulator (the same --grid-* and --carve-* options) and writes the frontier as
connected clusters (--cluster-connect 6|26, --cluster-min N voxels): origin, voxel, dims, the table (root, count, sum, lo, hi, tag),
n_all and from_root, with `from` at the pose of the last fuse: a cluster with tag == from_root can be reached through known-free space.

--eigen-products 3.3 fuses with the 3x3 products in the order of a reference built against Eigen >= 3.3
(DSM_FLAG_EIGEN33_PRODUCTS); the default, 3.2, is the order of Eigen 3.2, as without the flag.
"""
from __future__ import annotations

import argparse
import json

import numpy as np

from . import api, synth

_KIND = {"image": 0, "depth": 1, "orb": 2}


def write_log(path, cam, drift_free_poses, events):
    """events: the tuples of synth.node_messages."""
    with open(path, "wb") as f:
        f.write(np.array([cam.width, cam.height, drift_free_poses], "<i4").tobytes())
        f.write(np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.far, cam.near], "<f4").tobytes())
        for ev in events:
            kind = _KIND[ev[0]]
            f.write(np.array([kind], "<i4").tobytes() + np.array(ev[1], "<u4").tobytes())
            if kind == 0:
                f.write(np.ascontiguousarray(ev[2], "u1").tobytes())
            elif kind == 1:
                f.write(np.ascontiguousarray(ev[2], "<f4").tobytes())
            else:
                values = np.ascontiguousarray(ev[2], "<f4")
                path_poses = np.ascontiguousarray(ev[3], "<f8").reshape(-1, 7)
                f.write(np.array([values.size], "<i4").tobytes() + values.tobytes())
                f.write(np.array([len(path_poses)], "<i4").tobytes() + path_poses.tobytes())
                f.write(np.ascontiguousarray(ev[4], "<f8").tobytes() + np.ascontiguousarray(ev[5], "<f8").tobytes())
        f.write(np.array([-1], "<i4").tobytes())


def read_log(path):
    """Returns (camera, drift_free_poses, iterator over event tuples)."""
    f = open(path, "rb")

    def take(dtype, n=1):
        a = np.frombuffer(f.read(np.dtype(dtype).itemsize * n), dtype=dtype)
        if a.size != n:
            raise EOFError(f"{path}: truncated log")
        return a

    w, h, dfp = (int(v) for v in take("<i4", 3))
    fx, fy, cx, cy, far, near = (float(v) for v in take("<f4", 6))
    cam = synth.Camera(w, h, fx, fy, cx, cy, far=far, near=near)

    def events():
        while True:
            kind = int(take("<i4")[0])
            if kind < 0:
                f.close()
                return
            stamp = tuple(int(v) for v in take("<u4", 2))
            if kind == 0:
                yield ("image", stamp, take("u1", w * h).reshape(h, w))
            elif kind == 1:
                yield ("depth", stamp, take("<f4", w * h).reshape(h, w))
            else:
                values = take("<f4", int(take("<i4")[0]))
                path_poses = take("<f8", 7 * int(take("<i4")[0])).reshape(-1, 7)
                yield ("orb", stamp, values, path_poses, take("<f8", 7), take("<f8", 36))

    return cam, dfp, events()


def yaw_poses(pose, n) -> np.ndarray:
    """`pose` (4x4 cam -> world) turned about its own camera y axis by 2 pi k / n, k = 0 .. n - 1: float32 [n, 4, 4], made in double and
    rounded once (poses are inputs: what is scored is exactly what is returned)"""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    out = np.zeros((int(n), 4, 4), np.float32)
    for k in range(int(n)):
        a = 2.0 * np.pi * k / int(n)
        R = np.eye(4)
        R[0, 0], R[0, 2], R[2, 0], R[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
        out[k] = (T @ R).astype(np.float32)
    return out


EIGEN_PRODUCTS = {"3.2": 0, "3.3": api.DSM_FLAG_EIGEN33_PRODUCTS}  # --eigen-products -> SurfelMap(engine_flags=...)


def replay(path, save_cloud=None, save_mesh=None, device=0, surfel_capacity=0, eigen_products="3.2", save_mesh_binary=None, render=None, align=None,
           save_grid=None, grid_voxel=0.1, grid_dims=(64, 64, 32), grid_inflate=0, save_field=None, field_max_dist=16,
           save_space=None, carve_near=None, carve_far=None, carve_margin=None, save_frontier_clusters=None, cluster_min=1, cluster_connect=26,
           save_view_gain=None, view_yaws=8):
    """Feed a log to a SurfelMap on the GPU; returns a summary dict.  align = a cloud kind: after every fused frame that frame is
    aligned against the surfels of that kind at the pose it was fused with (SurfelMap.align_last, the library's defaults) and a
    JSON line says how it went; the poses fed to the map are not changed.  save_grid: the whole map as an occupancy grid of grid_dims voxels
    of grid_voxel metres around the final fuse pose (SurfelMap.grid), as an .npz.  save_field: the distance field of that grid's occupied
    set out to field_max_dist voxels (SurfelMap.field), as an .npz.  save_space: the free-space accumulator is switched on before the
    replay, in a grid of grid_dims voxels around the first pose of the log, and the three-state map and its frontier are written as an
    .npz (SurfelMap.set_free_space / space).  save_frontier_clusters: with the same accumulator, the frontier as clusters of
    cluster_connect-connectivity with at least cluster_min voxels, and whether each can be reached through known-free space from the
    pose of the last fuse (SurfelMap.frontier_clusters), as an .npz.  save_view_gain: with the same accumulator, view_yaws candidate
    poses -- the pose of the last fuse turned about its own camera y axis by 2 pi k / view_yaws (yaw_poses) -- scored by what the
    node's camera would see from each (SurfelMap.view_gain, the frontier as target), as an .npz with the poses, the scores and the
    camera."""
    from . import surfel_map
    cam, dfp, events = read_log(path)
    node = surfel_map.SurfelMap(cam, drift_free_poses=dfp, device=device, surfel_capacity=surfel_capacity,
                                engine_flags=EIGEN_PRODUCTS[eigen_products])
    if save_space or save_frontier_clusters or save_view_gain:  # (the node turns the SLAM frame so that the first camera sits at the world's origin: the grid lies around it)
        carve = {k: v for k, v in (("near_dist", carve_near), ("far_dist", carve_far), ("margin", carve_margin)) if v is not None}
        node.set_free_space(api.grid_spec_around((0.0, 0.0, 0.0), grid_voxel, tuple(grid_dims)), carve)
    n = 0
    for ev in events:
        fused = node.frames_fused
        node.feed(ev)
        n += 1
        if align and node.frames_fused > fused:
            a = node.align_last(align)
            T = a["T"].astype(np.float64)
            turn = 2.0 * np.arcsin(min(np.linalg.norm(T[:3, :3] - np.eye(3)) / np.sqrt(8.0), 1.0))
            print(json.dumps({"frame": node.frames_fused, "align": align, "status": api.ALIGN_STATUS[a["status"]], "iterations": a["iterations"],
                              "n_pixels": a["n_pixels"], "rms_m": a["rms"], "correction_m": float(np.linalg.norm(T[:3, 3])),
                              "correction_deg": float(np.degrees(turn))}))
    out = {"messages": n, "frames_fused": node.frames_fused, "keyframes": node.pose_count,
           "active_surfels": int(len(node.local_surfels())), "inactive_surfels": int(len(node.inactive_cloud()))}
    if save_cloud:
        node.save_cloud(save_cloud)
    if save_mesh:
        node.save_mesh(save_mesh)
    if save_mesh_binary:
        node.save_mesh_binary(save_mesh_binary)
    if render:  # the whole map as the node's camera sees it from the final fuse pose
        planes = node.render("all")
        np.savez(render, **{k: planes[k] for k in api.RENDER_PLANES})
    if save_grid:  # the whole map as a voxel grid around the final fuse pose
        g = node.grid("all", voxel=grid_voxel, dims=tuple(grid_dims), inflate=grid_inflate)
        sp = g["spec"]
        np.savez(save_grid, origin=np.array(sp.origin[:], np.float32), voxel=np.float32(sp.voxel), dims=np.array([sp.nx, sp.ny, sp.nz], np.int32),
                 inflate=np.int32(sp.inflate), occupied=g["occupied"], inflated=g["inflated"], cells=g["cells"])
        out["grid_cells"] = int(g["n_cells"])
    if save_field:  # the distance field of the same grid's occupied set
        f = node.field("all", voxel=grid_voxel, dims=tuple(grid_dims), max_dist=field_max_dist)
        sp = f["spec"]
        np.savez(save_field, origin=np.array(sp.origin[:], np.float32), voxel=np.float32(sp.voxel), dims=np.array([sp.nx, sp.ny, sp.nz], np.int32),
                 max_dist=np.int32(field_max_dist), dist2=f["dist2"], nearest=f["nearest"], distance=f["distance"])
        out["field_near"] = int((f["dist2"] != api.FIELD_FAR).sum())
    if save_space:  # the three states and the frontier of the accumulator's grid
        sp = node.space("all")
        free, n_free = node.free_space()
        g, p = sp["spec"], api.carve_params(carve)
        np.savez(save_space, origin=np.array(g.origin[:], np.float32), voxel=np.float32(g.voxel), dims=np.array([g.nx, g.ny, g.nz], np.int32),
                 near=np.float32(p.near_dist), far=np.float32(p.far_dist), margin=np.float32(p.margin), state=sp["state"], frontier_cells=sp["cells"],
                 free=free, n_free=np.int64(n_free), resets=np.int64(node.free_space_resets))
        out["free_voxels"], out["frontier_cells"], out["free_space_resets"] = int(n_free), int(sp["n_frontier"]), node.free_space_resets
    if save_frontier_clusters:  # the frontier as clusters, reachability from the pose of the last fuse
        origin = node.last_pose()[:3, 3]
        fc = node.frontier_clusters("all", connectivity=cluster_connect, min_count=cluster_min, origin=origin)
        g = fc["spec"]
        np.savez(save_frontier_clusters, origin=np.array(g.origin[:], np.float32), voxel=np.float32(g.voxel), dims=np.array([g.nx, g.ny, g.nz], np.int32),
                 connectivity=np.int32(cluster_connect), min_count=np.int32(cluster_min), table=fc["table"], from_root=np.int32(fc["from_root"]),
                 n_all=np.int32(fc["n_all"]), origin_point=np.asarray(origin, np.float32))
        out["frontier_clusters"], out["frontier_clusters_all"] = int(len(fc["table"])), int(fc["n_all"])
        out["frontier_clusters_reachable"] = int((fc["table"]["tag"] == fc["from_root"]).sum()) if fc["from_root"] >= 0 else 0
    if save_view_gain:  # the last pose turned about its own y axis: what would the node's camera see from each?
        poses = yaw_poses(node.last_pose(), view_yaws)
        q = node.view_query()
        scores = node.view_gain(poses, "all", camera=q.camera, target="frontier")
        g = node._space_spec
        np.savez(save_view_gain, origin=np.array(g.origin[:], np.float32), voxel=np.float32(g.voxel), dims=np.array([g.nx, g.ny, g.nz], np.int32),
                 poses=poses, scores=scores, camera=np.array([getattr(q.camera, f[0]) for f in api._RenderCamera._fields_], np.float64))
        out["view_poses"], out["view_best_yaw"] = int(len(poses)), int(np.argmax(scores["unknown"]))
        out["view_unknown_seen"] = [int(v) for v in scores["unknown"]]
    node.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("log")
    ap.add_argument("--save-cloud", help="ASCII PCD (SurfelMap::save_cloud)")
    ap.add_argument("--save-mesh", help="ASCII PLY hexagon mesh (SurfelMap::save_mesh)")
    ap.add_argument("--save-mesh-binary", help="the same mesh as a binary little-endian PLY, vertices built on the GPU")
    ap.add_argument("--render", metavar="PATH.npz", help="depth, index, normal and intensity images of the whole map at the final fuse pose")
    ap.add_argument("--align", metavar="KIND", choices=("active", "inactive", "all", "neighbor"),
                    help="after every fused frame, align it against the surfels of this cloud kind and print status, iterations, pixels, rms and the size of the correction")
    ap.add_argument("--save-grid", metavar="PATH.npz", help="the whole map as an occupancy voxel grid around the final fuse pose: origin, voxel, dims, "
                    "inflate, the occupied and inflated bit sets [nz][ny][(nx + 31) / 32] and the linear indices of the occupied cells")
    ap.add_argument("--grid-voxel", type=float, default=0.1, metavar="V", help="voxel edge in metres (default 0.1)")
    ap.add_argument("--grid-dims", type=int, nargs=3, default=(64, 64, 32), metavar=("NX", "NY", "NZ"), help="voxels per axis (default 64 64 32)")
    ap.add_argument("--grid-inflate", type=int, default=0, metavar="R", help="inflation radius in voxels, 0..16 (default 0)")
    ap.add_argument("--save-field", metavar="PATH.npz", help="the truncated Euclidean distance field of the occupied set of the --grid-voxel / --grid-dims "
                    "grid around the final fuse pose: origin, voxel, dims, max_dist and the planes dist2, nearest, distance [nz][ny][nx]")
    ap.add_argument("--field-max-dist", type=int, default=16, metavar="R", help="truncation radius of --save-field in voxels, 1..64 (default 16)")
    ap.add_argument("--save-space", metavar="PATH.npz", help="accumulate free space from every fused frame in the --grid-voxel / --grid-dims grid around the "
                    "first pose: origin, voxel, dims, state [nz][ny][nx] (0 unknown, 1 free, 2 occupied), frontier_cells, free, n_free, resets")
    ap.add_argument("--carve-near", type=float, default=None, metavar="N", help="nearest depth carved, metres (default: the library's, 0.1)")
    ap.add_argument("--carve-far", type=float, default=None, metavar="F", help="farthest depth carved, metres (default: the library's, 10)")
    ap.add_argument("--carve-margin", type=float, default=None, metavar="M", help="clearance kept in front of the measured surface, metres "
                    "(default: the library's, one voxel diagonal of a 0.1 m grid)")
    ap.add_argument("--save-frontier-clusters", metavar="PATH.npz", help="with the accumulator of --save-space (the same --grid-* and --carve-* options): the "
                    "frontier as connected clusters: origin, voxel, dims, table (root, count, sum, lo, hi, tag), from_root, n_all; from = the pose of the last fuse")
    ap.add_argument("--cluster-min", type=int, default=1, metavar="N", help="clusters of fewer voxels are left out (default 1)")
    ap.add_argument("--cluster-connect", type=int, default=26, choices=(6, 26), help="connectivity of the clusters (default 26)")
    ap.add_argument("--save-view-gain", metavar="PATH.npz", help="with the accumulator of --save-space (the same --grid-* and --carve-* options): --view-yaws "
                    "poses, the last fused pose turned about its own camera y axis, scored by what the node's camera would see: origin, voxel, dims, poses, "
                    "scores (in_view, visible, unknown, free, occupied, target = frontier), camera")
    ap.add_argument("--view-yaws", type=int, default=8, metavar="N", help="number of yaw poses of --save-view-gain, 1..4096 (default 8)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--eigen-products", choices=sorted(EIGEN_PRODUCTS), default="3.2",
                    help="product order of the Eigen the reference to match was built against (3.3: Eigen 3.3 / 3.4)")
    ap.add_argument("--synth", type=int, metavar="N", help="first write LOG: N frames of the synthetic circuit at 1226x370")
    args = ap.parse_args()
    if args.synth:
        cam = synth.KITTI_1226
        write_log(args.log, cam, 10, synth.node_messages(cam, synth.Scene(), args.synth, lap=120))
    print(json.dumps(replay(args.log, args.save_cloud, args.save_mesh, device=args.device, eigen_products=args.eigen_products,
                            save_mesh_binary=args.save_mesh_binary, render=args.render, align=args.align,
                            save_grid=args.save_grid, grid_voxel=args.grid_voxel, grid_dims=args.grid_dims, grid_inflate=args.grid_inflate,
                            save_field=args.save_field, field_max_dist=args.field_max_dist,
                            save_space=args.save_space, carve_near=args.carve_near, carve_far=args.carve_far, carve_margin=args.carve_margin,
                            save_frontier_clusters=args.save_frontier_clusters, cluster_min=args.cluster_min, cluster_connect=args.cluster_connect,
                            save_view_gain=args.save_view_gain, view_yaws=args.view_yaws)))


if __name__ == "__main__":
    main()
