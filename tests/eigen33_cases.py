"""Shared by tests/golden/make_golden_eigen33.py and the Eigen >= 3.3 product-order tests: the cases the fixtures of
tests/golden/eigen33_golden.json were recorded on, and the digests they store."""
import hashlib

import numpy as np

# The synthetic trajectories (densesurfelmapping_amd/synth.py) turn about the vertical axis only: every row of their
# rotations has a zero, and a0*b0 + (a1*b1 + a2*b2) == (a0*b0 + a1*b1) + a2*b2 whenever one of the three terms is zero.  Both
# Eigen orders give the same bits on them.  The fixtures therefore see the same scenes from a world frame tilted about an
# oblique axis: pose -> WORLD @ pose (the frames are rendered from the untilted scene; a rigid change of world coordinates).


def _rigid(axis, angle, t) -> np.ndarray:
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    m[:3, 3] = t
    return m


WORLD = _rigid([0.3, -0.5, 0.8], 0.4, [0.3, -0.2, 0.5])


def tilt(pose) -> np.ndarray:
    """cam->world 4x4 float32 in the tilted world frame"""
    return (WORLD @ np.asarray(pose, np.float64)).astype(np.float32)


# the synthetic sequences, fused frame by frame from an empty map with tilted poses
SEQUENCES = [
    {"name": "tiny_40", "camera": "TINY", "scene": {"seed": 12345}, "frames": 40},
    {"name": "tiny_ragged_40", "camera": "TINY_RAGGED", "scene": {"seed": 77}, "frames": 40},
    {"name": "kitti1226_24", "camera": "KITTI_1226", "scene": {"seed": 12345}, "frames": 24},
    {"name": "vga_rgbd_8", "camera": "VGA_RGBD", "scene": {"seed": 5, "scale": 0.12, "step": 0.05}, "frames": 8},
]


def sequence(case, synth):
    """synth.sequence of a SEQUENCES case with tilted poses: (t, image, depth, pose, ref_idx)"""
    cam = getattr(synth, case["camera"])
    for t, img, dep, pose, ridx in synth.sequence(cam, synth.Scene(**case["scene"]), case["frames"]):
        yield t, img, dep, tilt(pose), ridx


# the hostile frames of tests/test_gpu_parity.py:edge_cases at these sizes: each fused twice, ref_idx 0 from an empty map
# under EDGE_POSES[0], then ref_idx 1 over the map it made under EDGE_POSES[1] (a slightly different view, so that the
# fusion's products meet normals that are not a column of the rotation)
EDGE_CAMERAS = ["TINY_RAGGED", "KITTI_1226"]
EDGE_POSES = [WORLD.astype(np.float32), (WORLD @ _rigid([-0.7, 0.2, 0.4], 0.03, [0, 0, 0])).astype(np.float32)]

# the node scenario of tests/node_state.SCENARIOS that is recorded, with its poses tilted
NODE_SCENARIO = "circuit_60"


class _TiltedScene:
    def __init__(self, scene):
        self.scene = scene

    def pose(self, t):
        return tilt(self.scene.pose(t))


def run_node(make_node, synth, node_state):
    """make_node_golden.run_case for NODE_SCENARIO in the tilted world: (briefs, checkpoints, final snapshot, file digests)"""
    import os
    import tempfile
    case = next(c for c in node_state.SCENARIOS if c["name"] == NODE_SCENARIO)
    cam, scene = node_state.camera_and_scene(case, synth)
    kw = dict(case["kw"])
    kw["frames"] = {tl: synth.render(cam, scene, tl)[:2] for tl in range(kw.get("lap", 40))}
    node = make_node(cam, case["drift_free_poses"])
    briefs, checkpoints = [], {}
    for ev in synth.node_messages(cam, _TiltedScene(scene), case["frames"], **kw):
        node.feed(ev)
        if ev[0] == "orb":
            briefs.append(node_state.brief(node))
            if len(briefs) % 10 == 0:
                checkpoints[str(len(briefs))] = node_state.digest(node_state.snapshot(node))
    final = node_state.snapshot(node)
    with tempfile.TemporaryDirectory() as td:
        pcd, ply = os.path.join(td, "map.PCD"), os.path.join(td, "map_mesh.PLY")
        node.save_cloud(pcd)
        node.save_mesh(ply)
        files = {"pcd": node_state.file_digest(pcd), "ply": node_state.file_digest(ply)}
    node.close()
    return briefs, checkpoints, final, files


def canon_field(x: np.ndarray) -> bytes:
    x = np.ascontiguousarray(x)
    if x.dtype.kind == "f":
        x = x.copy()
        x[np.isnan(x)] = np.nan  # one canonical NaN: sign / payload are not defined by the reference's arithmetic
    return x.tobytes()


def fields_digest(a: np.ndarray) -> str:
    """sha256 over the fields of a structured array, field by field (no padding bytes), NaN canonical."""
    h = hashlib.sha256()
    for f in a.dtype.names:
        h.update(f.encode())
        h.update(canon_field(a[f]))
    return h.hexdigest()


def frame_record(n_new, local, labels, seeds) -> dict:
    return {"n_new": int(n_new), "n_local": int(len(local)), "labels_sha256": hashlib.sha256(np.ascontiguousarray(labels).tobytes()).hexdigest(),
            "seeds_sha256": fields_digest(seeds), "map_sha256": fields_digest(local)}


# final maps larger than this are recorded by digest (fields_digest) only, to keep the fixtures small
MAX_STORED_MAP_BYTES = 512 * 1024


def final_map_differences(got: np.ndarray, rec: dict, golden_dir: str) -> list:
    """[] when `got` is the final map of a sequence fixture `rec` bit for bit (NaN == NaN), else what differs: the fields
    (fields_equal's form) where the map is stored, ["digest"] where only its digest is"""
    import os
    if len(got) != rec["final_n"]:
        return [("len", abs(len(got) - rec["final_n"]))]
    if rec["final_map"] is None:
        return [] if fields_digest(got) == rec["final_sha256"] else ["digest"]
    want = np.load(os.path.join(golden_dir, rec["final_map"]))
    bad = []
    for f in want.dtype.names:
        x, y = got[f], want[f]
        same = (x.view("u4") == y.view("u4")) | (np.isnan(x) & np.isnan(y)) if x.dtype.kind == "f" else x == y
        if not same.all():
            bad.append((f, int((~same).sum())))
    return bad


def rows_differing(a: np.ndarray, b: np.ndarray) -> int:
    """records of two maps that differ in any bit (NaN == NaN); surplus records of the longer map count as differing"""
    n = min(len(a), len(b))
    bad = np.zeros(n, bool)
    for f in a.dtype.names:
        x, y = a[f][:n], b[f][:n]
        if x.dtype.kind == "f":
            bad |= ~((x.view("u4") == y.view("u4")) | (np.isnan(x) & np.isnan(y)))
        else:
            bad |= x != y
    return int(bad.sum()) + abs(len(a) - len(b))
