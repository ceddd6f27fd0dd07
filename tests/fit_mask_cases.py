"""Case builders of tests/test_gpu_fit_masks.py: small sequences for batches of eight handles, their replay through the C
restatement (PortOracle) with every frame's state kept, and a host census of which seeds get a plane (the m_in > 0 contract
of the inlier row masks, DeviceCtx::inl_mask)."""
import concurrent.futures

import numpy as np

B = 8          # handles per batch: the smallest batch that takes the lane-per-seed forms
N_FRAMES = 4   # one frame group of four


def tight_camera(synth):
    """166x103's ragged height with a width that IS its pitch (a multiple of 64): S = 24 x 12 = 288, still no multiple of 64"""
    return synth.Camera(192, 103, 120.0, 120.0, 95.5, 51.0)


def batch_runs(synth, cam, n_frames=N_FRAMES, first_seed=40, **scene_kw):
    """runs[b] = [(image, depth, pose, ref)]: handle b sees its own scene"""
    return [[(img, dep, pose, ref) for _, img, dep, pose, ref in synth.sequence(cam, synth.Scene(seed=first_seed + b, **scene_kw), n_frames)]
            for b in range(B)]


def oracle_replay(ob, cam, frames, eigen33=False):
    """one PortOracle through the frames: per frame (new count, label image, seed table, map), copies"""
    orc = ob.PortOracle(cam, eigen33=eigen33)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    recs = []
    for img, dep, pose, ref in frames:
        lo, k = orc.fuse_map(ref, img, dep, pose, lo)
        recs.append((k, orc.labels().copy(), orc.seeds().copy(), lo.copy()))
    return recs


def oracle_replays(ob, cam, runs, eigen33=False):
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(runs)) as ex:
        return list(ex.map(lambda fr: oracle_replay(ob, cam, fr, eigen33), runs))


def plane_census(labels, depth, seeds, huber=0.4):
    """Per seed, from a frame's final label image and seed table (FF.cpp:811-862 spelled in numpy): members with depth > 0.05,
    depth inliers of the seed's mean depth among them, and whether the seed gets a plane (>= 16 with depth, >= 80 % inliers)."""
    S = len(seeds)
    lab = labels.astype(np.int64).ravel()
    d = depth.astype(np.float32).ravel()
    member = lab >= 0
    md = seeds["mean_depth"].astype(np.float32)[np.where(member, lab, 0)]
    has_depth = member & (d.astype(np.float64) > 0.05)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (md - d).astype(np.float32).astype(np.float64)
    inlier = has_depth & (r < huber) & (r > -huber)
    n = np.bincount(lab[has_depth], minlength=S)
    m = np.bincount(lab[inlier], minlength=S)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = (m.astype(np.float32) / n.astype(np.float32)).astype(np.float64)
    fitted = (n >= 16) & ~(ratio < 0.8)
    return n, m, fitted


def has_plane(seeds):
    """as the reference itself asks (FF.cpp:321): a seed without a plane keeps the zero normal"""
    return (seeds["norm_x"] != 0) | (seeds["norm_y"] != 0) | (seeds["norm_z"] != 0)
