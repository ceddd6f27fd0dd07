"""Caller-supplied pose inverses (the *_inv entry points of include/dsm.h, FF.cpp:59) for the parity tests of
tests/test_cpu.py and tests/test_gpu_inverse.py.  Every inverse is 16 float32, column-major (an Eigen::Matrix4f's storage),
generated from a fixed seed.  Three families:

  * "near"    -- the closed form (oracle/dsm_oracle.c inverse4f) moved by -2 .. +2 ulps per element, a different pattern
                 per frame (what another Eigen build would hand over);
  * "wrong"   -- the exact inverse of the pose shifted by a few centimetres or turned by a few tenths of a degree: counts
                 and delete decisions change, so a form that ignores the inverses cannot pass;
  * "hostile" -- the closed form, except on a few frames: a NaN element, an inf element, a singular matrix.  The reference
                 uses whatever it is given, and so does the engine; the expected map is whatever the C restatement makes of it.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("near", "wrong", "hostile")


def _port():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "liboracle_port.so"))
    lib.dsmo_inverse4f.argtypes = [C.c_void_p, C.c_void_p]
    return lib


def colmajor(m):
    return np.ascontiguousarray(np.asarray(m, np.float32).T).ravel()


def closed_form(pose):
    """the library's own inverse of a 4x4 row-major cam->world pose (adjugate / determinant), column-major"""
    p = colmajor(pose)
    out = np.zeros(16, np.float32)
    _port().dsmo_inverse4f(p.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def ulp_move(a, ulps):
    """float32 array `a` with element i moved by ulps[i] units in the last place (towards +inf for > 0)"""
    a = np.array(a, np.float32)
    for i, k in enumerate(np.asarray(ulps).ravel()):
        for _ in range(abs(int(k))):
            a[i] = np.nextafter(a[i], np.float32(np.inf if k > 0 else -np.inf))
    return a


def ulp_pattern(rng):
    """16 ulp offsets in [-2, 2], at least one non-zero in the rows the fusion reads (rows 0-2 of the matrix)"""
    while True:
        u = rng.integers(-2, 3, 16).astype(np.int32)
        if np.any(u.reshape(4, 4)[:, :3] != 0):  # (column-major: [:, :3] of the reshape are rows 0-2 of every column)
            return u


def _nudged(pose, t, rng):
    """pose (row-major, cam->world) shifted by 2-4 cm or turned by 0.2-0.5 degrees about a random axis, in float64"""
    m = np.asarray(pose, np.float64).copy()
    if t % 2 == 0:
        d = rng.normal(size=3)
        m[:3, 3] += d / np.linalg.norm(d) * rng.uniform(0.02, 0.04)
    else:
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        a = np.deg2rad(rng.uniform(0.2, 0.5))
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
        m[:3, :3] = m[:3, :3] @ R
    return m


def hostile_kind(t):
    """which frames of a sequence get a hostile inverse in the "hostile" family: a few of every eleven"""
    return {3: "nan", 6: "inf", 9: "singular"}.get(t % 11)


def inverses(family, poses, seed):
    """[n, 16] float32 column-major caller inverses of the given family for the row-major poses [n, 4, 4]"""
    rng = np.random.default_rng(seed)
    out = []
    for t, pose in enumerate(poses):
        base = closed_form(pose)
        if family == "near":
            inv = ulp_move(base, ulp_pattern(rng))
        elif family == "wrong":
            inv = colmajor(np.linalg.inv(_nudged(pose, t, rng)))
        elif family == "hostile":
            inv = base.copy()
            kind = hostile_kind(t)
            r, c = int(rng.integers(0, 3)), int(rng.integers(0, 4))  # an element of rows 0-2 (the ones the fusion reads)
            if kind == "nan":
                inv[4 * c + r] = np.nan
            elif kind == "inf":
                inv[4 * c + r] = np.inf if rng.random() < 0.5 else -np.inf
            elif kind == "singular":  # the rotation's second column zeroed: world y no longer moves anything
                inv[4:7] = 0.0
        else:
            raise ValueError(family)
        out.append(inv)
    return np.stack(out).astype(np.float32)
