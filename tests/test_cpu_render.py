"""The map renderer's definition without a GPU: csrc/dsm_math.h's render_setup / render_hit / render_key through the two host
renderers of tests/render_host.cpp (the checker tests/test_gpu_render.py compares the kernels with, bit for bit).
  1. boxed == brute: the early rejects and the pixel box lose no hit, for any record
  2. exact dyadic scenes against a numpy float64 restatement written here
  3. generic surfels against that restatement, where its own margins are clear
  4. the declarations
  5. render_host.cpp's own main under the sanitizers"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dtype():
    from densesurfelmapping_amd import api
    return api.SURFEL_DTYPE


def _boxed_is_brute(s, cam, pose, what):
    for flags in (0, rc.CULL_BACKFACES):
        for e33 in (False, True):
            boxed = rc.host_render(s, cam, pose, flags=flags, eigen33=e33, brute=False)
            brute = rc.host_render(s, cam, pose, flags=flags, eigen33=e33, brute=True)
            rc.same_planes(boxed, brute, (what, cam.width, flags, e33))
    return brute


# ------------------------------------------------------------------ 1. boxed == brute
def test_boxed_equals_brute_crafted(dtype):
    for cam in (rc.CAM_48, rc.CAM_70, rc.CAM_96):
        s, names = rc.crafted_records(dtype, cam)
        for pose in (rc.IDENTITY, rc.oblique_pose()):
            out = _boxed_is_brute(s, cam, pose, "crafted")
        assert (out["index"] >= 0).any()
    # at the identity pose the crafted set shows what it is meant to show
    s, names = rc.crafted_records(dtype, rc.CAM_70)
    out = rc.host_render(s, rc.CAM_70, rc.IDENTITY)
    seen = set(np.unique(out["index"]).tolist())
    for name in ("fronto-parallel", "tilted", "left border", "right border", "top border", "bottom border", "corner", "negative size",
                 "straddles the near plane", "straddles the far plane", "covers the whole image", "duplicate a", "update_times 0", "size 0",
                 "the camera centre inside a disc's reach: the plane x = 2.5", "colour NaN"):
        assert names.index(name) in seen, name
    for name in ("zero normal", "behind the camera", "NaN size", "NaN position", "inf position", "size 0 off the rays", "duplicate b", "wholly outside, left",
                 "the camera centre in the disc's plane, exactly", "edge-on through the centre: denominator 0 on its column"):
        assert names.index(name) not in seen, name
    assert (out["index"] >= 0).all()  # ("covers the whole image" does)


def test_boxed_equals_brute_random(dtype):
    rng = np.random.default_rng(2024)
    sets = (("random bits", mc.random_records(rng, 2000, dtype)), ("plausible", mc.plausible_records(rng, 2000, dtype)),
            ("visible", rc.render_records(rng, 2000, dtype)))
    for cam in (rc.CAM_48, rc.CAM_70):
        for what, s in sets:
            for pose in (rc.IDENTITY, rc.oblique_pose()):
                out = _boxed_is_brute(s, cam, pose, what)
            if what == "visible":
                assert (out["index"] >= 0).mean() > 0.5


def test_boxes_stay_inside_the_image(dtype):
    rng = np.random.default_rng(5)
    s = np.concatenate([mc.random_records(rng, 3000, dtype), rc.crafted_records(dtype)[0], rc.render_records(rng, 500, dtype)])
    for cam in (rc.CAM_48, rc.CAM_96):
        box, keep = rc.host_boxes(s, cam, rc.oblique_pose())
        b = box[keep]
        assert keep.any()
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 2] <= cam.width).all() and (b[:, 3] <= cam.height).all()
        assert (b[:, 0] < b[:, 2]).all() and (b[:, 1] < b[:, 3]).all()


# ------------------------------------------------------------------ the float64 restatement (2, 3)
def np_render64(s, cam, pose, flags=0):
    """The definition of include/dsm.h in numpy float64 from the float32 inputs.  Per pixel: the winner's number (-1: none) and
    depth, and `clear`: no surfel's decision at the pixel is within 1e-4 of flipping -- |dist^2 - r^2| > 1e-4 r^2, |denominator| >
    1e-4 (or the depth it gives is beyond the far plane whatever its error), z more than 1e-4 relative from both planes -- and
    the runner-up is more than 1e-4 relative behind the winner."""
    f64 = np.float64
    P = np.asarray(pose, np.float32).astype(f64)
    inv = np.linalg.inv(P)
    pw = np.stack([s["px"], s["py"], s["pz"]], 1).astype(f64)
    nw = np.stack([s["nx"], s["ny"], s["nz"]], 1).astype(f64)
    pc = pw @ inv[:3, :3].T + inv[:3, 3]
    nc = nw @ inv[:3, :3].T
    d = (nc * pc).sum(1)
    r2 = s["size"].astype(f64) ** 2
    near, far = f64(cam.near_dist), f64(cam.far_dist)
    RX, RY = np.meshgrid((np.arange(cam.width, dtype=f64) - f64(cam.cx)) / f64(cam.fx), (np.arange(cam.height, dtype=f64) - f64(cam.cy)) / f64(cam.fy))
    best = np.full(RX.shape, np.inf)
    second = np.full(RX.shape, np.inf)
    index = np.full(RX.shape, -1, np.int64)
    unclear = np.zeros(RX.shape, bool)
    with np.errstate(all="ignore"):
        for i in range(len(s)):
            if (flags & rc.CULL_BACKFACES) and d[i] >= 0:
                continue
            den = nc[i, 0] * RX + nc[i, 1] * RY + nc[i, 2]
            z = d[i] / den
            small_den = np.abs(den) <= 1e-4
            beyond = small_den & (abs(d[i]) > 1e-4 * far * 1.001)  # |z| >= |d| / 1e-4 > far
            dist2 = (z * RX - pc[i, 0]) ** 2 + (z * RY - pc[i, 1]) ** 2 + (z - pc[i, 2]) ** 2
            out_of_range = ~small_den & ((z < near * (1 - 1e-4)) | (z > far * (1 + 1e-4)))
            in_range = ~small_den & (z > near * (1 + 1e-4)) & (z < far * (1 - 1e-4))
            miss = beyond | out_of_range | (in_range & (dist2 > r2[i] * (1 + 1e-4)))
            unclear |= ~(miss | (in_range & (dist2 < r2[i] * (1 - 1e-4))))
            hit = np.isfinite(z) & (z > near) & (z < far) & (dist2 <= r2[i])  # the definition itself
            closer = hit & (z < best)
            second = np.where(closer, best, np.where(hit & (z < second), z, second))
            index = np.where(closer, i, index)
            best = np.where(closer, z, best)
    clear = ~unclear & ~((index >= 0) & (second <= best * (1 + 1e-4)))
    return index, np.where(index >= 0, best, 0.0), clear


DYADIC = rc.Camera(70, 37, 64.0, 64.0, 32.0, 16.0, 0.25, 16.0)


def _records(dtype, rows):
    a = np.zeros(len(rows), dtype)
    for i, r in enumerate(rows):
        base = dict(px=0.0, py=0.0, pz=2.0, nx=0.0, ny=0.0, nz=-1.0, size=0.25, color=100.0 + i, weight=1.0, update_times=7, last_update=0)
        base.update(r)
        for k, v in base.items():
            a[k][i] = v
    return a


def _exact(s, cam, pose=rc.IDENTITY, flags=0):
    """every figure of these scenes is dyadic: float32 and float64 agree exactly, no margins"""
    got = rc.host_render(s, cam, pose, flags=flags)
    index, depth, _ = np_render64(s, cam, pose, flags)
    assert np.array_equal(got["index"], index)
    assert np.array_equal(got["depth"].astype(np.float64), depth)
    hit = index >= 0
    assert np.array_equal(got["intensity"][hit], np.clip(s["color"][index[hit]], 0, 255).astype(np.uint8)) and (got["intensity"][~hit] == 0).all()
    assert np.array_equal(got["normal"][hit], np.stack([s["nx"], s["ny"], s["nz"]], 1)[index[hit]]) and (got["normal"][~hit] == 0).all()
    return got


# ------------------------------------------------------------------ 2. exact dyadic cases
def test_dyadic_fronto_parallel_disc(dtype):
    got = _exact(_records(dtype, [{}]), DYADIC)
    v, u = np.mgrid[0:37, 0:70]
    inside = (u - 32) ** 2 + (v - 16) ** 2 <= 64
    assert np.array_equal(got["index"] == 0, inside) and inside.sum() == 197
    assert (got["depth"][inside] == 2.0).all() and (got["depth"][~inside] == 0.0).all() and (got["index"][~inside] == -1).all()


def _wall():
    return [dict(px=0.5 * i, py=0.5 * j, pz=4.0, size=0.5) for j in range(-3, 4) for i in range(-5, 7)]


def test_dyadic_disc_before_a_wall(dtype):
    wall = _wall()
    s = _records(dtype, wall + [{}])  # the near disc has the HIGHEST number: depth decides, not the number
    got = _exact(s, DYADIC)
    v, u = np.mgrid[0:37, 0:70]
    inside = (u - 32) ** 2 + (v - 16) ** 2 <= 64
    assert (got["index"][inside] == len(wall)).all() and (got["depth"][inside] == 2.0).all()
    assert (got["depth"][~inside] == 4.0).all() and (got["index"][~inside] >= 0).all() and (got["index"][~inside] < len(wall)).all()
    # the wall's surfels overlap at one depth: the lowest number covering a pixel shows
    x, y = (u - 32) / 64.0 * 4.0, (v - 16) / 64.0 * 4.0
    lowest = np.full(u.shape, -1)
    for k in reversed(range(len(wall))):
        lowest = np.where((x - wall[k]["px"]) ** 2 + (y - wall[k]["py"]) ** 2 <= 0.25, k, lowest)
    assert np.array_equal(got["index"][~inside], lowest[~inside])


def test_dyadic_identical_records(dtype):
    s = _records(dtype, [dict(px=3.0, py=3.0), {}, {}, dict(px=-3.0)])  # 1 and 2 are the same surfel (but for the colour)
    got = _exact(s, DYADIC)
    assert (got["index"] == 1).sum() == 197 and not (got["index"] == 2).any()
    assert (got["intensity"][got["index"] == 1] == 101).all()


def test_dyadic_backface_cull(dtype):
    front, twin = {}, dict(nz=1.0)
    for rows, seen_default, seen_culled in (([twin], 197, 0), ([front], 197, 197), ([twin, front], 197, 197)):
        s = _records(dtype, rows)
        assert (_exact(s, DYADIC)["index"] >= 0).sum() == seen_default
        got = _exact(s, DYADIC, flags=rc.CULL_BACKFACES)
        assert (got["index"] >= 0).sum() == seen_culled
    both = _records(dtype, [twin, front])
    assert (_exact(both, DYADIC)["index"].max() == 0) and (_exact(both, DYADIC, flags=rc.CULL_BACKFACES)["index"].max() == 1)


# ------------------------------------------------------------------ 3. generic surfels
GENERIC_SEED = 11


def generic_scene(dtype, seed=GENERIC_SEED, n=300, cam=rc.CAM_96):
    """n surfels in the view of `cam` at oblique_pose(): footprints of at least three pixels, normals up to 75 degrees off the
    direction to the camera"""
    rng = np.random.default_rng(seed)
    pose = rc.oblique_pose()
    z = rng.uniform(0.6, 8.0, n)
    u, v = rng.uniform(0, cam.width - 1, n), rng.uniform(0, cam.height - 1, n)
    pc = np.stack([(u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z], 1)
    to_cam = -pc / np.linalg.norm(pc, axis=1, keepdims=True)
    tilt = np.radians(rng.uniform(0, 75, n))
    any_dir = rng.normal(size=(n, 3))
    side = np.cross(to_cam, any_dir)
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    nc = np.cos(tilt)[:, None] * to_cam + np.sin(tilt)[:, None] * side
    nc *= rng.choice([-1.0, 1.0], n)[:, None]  # two-sided
    P = pose.astype(np.float64)
    a = np.zeros(n, dtype)
    pw = pc @ P[:3, :3].T + P[:3, 3]
    nw = nc @ P[:3, :3].T
    for k, f in enumerate(("px", "py", "pz")):
        a[f] = pw[:, k]
    for k, f in enumerate(("nx", "ny", "nz")):
        a[f] = nw[:, k]
    # radius / depth >= 1.5 pixels / min(fx, fy) / cos(75 deg): the disc's short projected axis spans three pixels
    a["size"] = z * rng.uniform(1.5, 4.0, n) / min(cam.fx, cam.fy) / np.cos(np.radians(75))
    a["color"] = rng.uniform(0, 255, n)
    a["weight"] = 1.0
    a["update_times"] = 7
    return a, pose


def test_generic_surfels_against_float64(dtype):
    cam = rc.CAM_96
    s, pose = generic_scene(dtype)
    index, depth, clear = np_render64(s, cam, pose)
    covered = index >= 0
    left_out = (~clear).sum()
    print("generic scene: %d of %d pixels covered, %d left out (%.2f %% of the covered)" % (covered.sum(), covered.size, left_out, 100.0 * left_out / covered.sum()))
    assert covered.sum() > 0.5 * covered.size
    assert left_out <= 0.05 * covered.sum()  # the condition of the comparison, met by the restatement alone (GENERIC_SEED)
    got = rc.host_render(s, cam, pose)
    rc.same_planes(got, rc.host_render(s, cam, pose, brute=False), "generic")
    bad = clear & (got["index"] != index)
    assert not bad.any(), (bad.sum(), np.argwhere(bad)[0], got["index"][bad][0], index[bad][0])
    both = clear & covered
    rel = np.abs(got["depth"].astype(np.float64)[both] - depth[both]) / depth[both]
    print("largest relative depth difference %.3g" % rel.max())
    assert rel.max() <= 1e-5
    assert (got["depth"][clear & ~covered] == 0).all()
    # the normal and the intensity are the winner's
    want_n = np.stack([s["nx"], s["ny"], s["nz"]], 1).astype(np.float64) @ np.linalg.inv(pose.astype(np.float64))[:3, :3].T
    assert np.abs(got["normal"][both] - want_n[index[both]]).max() < 1e-5
    assert np.array_equal(got["intensity"][both], s["color"][index[both]].astype(np.int32).astype(np.uint8))


# ------------------------------------------------------------------ 4. declarations
def test_render_abi_declarations():
    from densesurfelmapping_amd import api, build, surfel_map
    build.build_library()
    lib = C.CDLL(api.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "dsm.h")).read()
    node_hdr = open(os.path.join(ROOT, "include", "dsm_surfel_map.h")).read()
    assert "dsm_render_compose" in api.ABI_SYMBOLS and "dsm_render_compose(" in hdr and hasattr(lib, "dsm_render_compose")
    for name in ("dsm_surfel_map_render", "dsm_surfel_map_render_device"):
        assert name in surfel_map.ABI_SYMBOLS and name + "(" in node_hdr and hasattr(lib, name), name
    assert re.search(r"#define DSM_ABI_VERSION 4\b", hdr)
    lib.dsm_abi_version.restype = C.c_int
    assert lib.dsm_abi_version() == 4
    assert re.search(r"#define DSM_RENDER_CULL_BACKFACES 1u", hdr) and api.RENDER_CULL_BACKFACES == 1 == rc.CULL_BACKFACES
    assert "typedef struct dsm_render_camera" in hdr and "typedef struct dsm_render_planes" in hdr
    assert C.sizeof(api._RenderCamera) == 32 == C.sizeof(rc.Camera) and C.sizeof(api._RenderPlanes) == 4 * C.sizeof(C.c_void_p)
    assert [f[0] for f in api._RenderCamera._fields_] == ["width", "height", "fx", "fy", "cx", "cy", "near_dist", "far_dist"]
    assert (surfel_map.CLOUD_ACTIVE, surfel_map.CLOUD_INACTIVE, surfel_map.CLOUD_ALL, surfel_map.CLOUD_NEIGHBOR, surfel_map.CLOUD_RAW) == (0, 1, 2, 3, 4)
    # without a handle every call is refused before anything else
    lib.dsm_render_compose.argtypes = [C.c_void_p, C.c_int, C.c_int32] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    assert lib.dsm_render_compose(None, 1, 0, None, None, None, None, None, 0, None, 0, None) == api.DSM_E_INVALID
    lib.dsm_surfel_map_render.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    assert lib.dsm_surfel_map_render(None, 0, None, None, 0, None, None) == api.DSM_E_INVALID
    hpp = open(os.path.join(ROOT, "include", "dsm_surfel_map.hpp")).read()
    assert "dsm_surfel_map_render(" in hpp and "dsm_surfel_map_render_device(" in hpp
    assert hasattr(api.FusionFunctions, "render") and hasattr(surfel_map.SurfelMap, "render")


# ------------------------------------------------------------------ 5. the stand-alone program under the sanitizers
def test_render_host_main_under_sanitizers(dtype, tmp_path):
    exe = str(tmp_path / "render_host_main")
    r = rc.build_main(exe)
    assert r.returncode == 0, r.stderr  # this g++ has -fsanitize=address,undefined and float-cast-overflow
    paths = []
    for k, cam in enumerate((rc.CAM_48, rc.CAM_70)):
        p = str(tmp_path / ("crafted%d.bin" % k))
        rc.crafted_records(dtype, cam)[0].tofile(p)
        paths.append(p)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    assert "boxed == brute" in r.stdout
