"""DSM_FLAG_EIGEN33_PRODUCTS without a GPU: the Eigen >= 3.3 stand-in (tests/eigen33/Eigen), the device product
xform_dir_e33 compiled for the host against it, the fixtures of tests/golden/make_golden_eigen33.py against the Eigen 3.2
order, and the C++ facades' choice of the flag."""
import ctypes as C
import difflib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, fields_equal

GOLDEN = os.path.join(ROOT, "tests", "golden")
SHIM = os.path.join(ROOT, "oracle", "shims", "Eigen")
STANDIN = os.path.join(ROOT, "tests", "eigen33", "Eigen")


def _gold():
    return json.load(open(os.path.join(GOLDEN, "eigen33_golden.json")))


def test_standin_differs_only_in_the_two_product_bodies():
    for name in ("Dense", "Geometry"):
        assert open(os.path.join(SHIM, name)).read() == open(os.path.join(STANDIN, name)).read(), name
    a = open(os.path.join(SHIM, "Eigen")).read().splitlines()
    b = open(os.path.join(STANDIN, "Eigen")).read().splitlines()
    assert len(a) == len(b)
    changed = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert len(changed) == 2, [a[i] for i in changed]
    want = {  # the 3.2 body -> the 3.3 body, for Block33 * Vector3 and Matrix3 * Vector3
        "    for (int i = 0; i < 3; i++) r(i) = (b.m[0 * 3 + i] * v(0) + b.m[1 * 3 + i] * v(1)) + b.m[2 * 3 + i] * v(2);":
        "    for (int i = 0; i < 3; i++) r(i) = b.m[0 * 3 + i] * v(0) + (b.m[1 * 3 + i] * v(1) + b.m[2 * 3 + i] * v(2));",
        "    for (int i = 0; i < 3; i++) r(i) = (a(i, 0) * v(0) + a(i, 1) * v(1)) + a(i, 2) * v(2);":
        "    for (int i = 0; i < 3; i++) r(i) = a(i, 0) * v(0) + (a(i, 1) * v(1) + a(i, 2) * v(2));",
    }
    assert {a[i]: b[i] for i in changed} == want, list(difflib.unified_diff(a, b, lineterm=""))
    heads = [a[i - 2] for i in changed]  # the operator* each body belongs to
    assert "operator*(const Block33<T> &b, const Matrix<T, 3, 1> &v)" in heads[0]
    assert "operator*(const Matrix<T, 3, 3> &a, const Matrix<T, 3, 1> &v)" in heads[1]


_PRODUCT_SRC = r"""
#include "dsm_math.h"
#include <Eigen/Eigen>
// m: column-major 4x4, v: 3 floats; out[0..2] = dsm::%(fn)s, out[3..5] = m.block<3,3>(0,0) * v, out[6..8] = Matrix3f * v
extern "C" void products(const float *m, const float *v, float *out, int n) {
    for (int k = 0; k < n; k++, m += 16, v += 3, out += 9) {
        dsm::%(fn)s(m, v, out);
        Eigen::Matrix<float, 4, 4> M;
        Eigen::Matrix<float, 3, 3> R;
        for (int j = 0; j < 4; j++)
            for (int i = 0; i < 4; i++) M(i, j) = m[j * 4 + i];
        for (int j = 0; j < 3; j++)
            for (int i = 0; i < 3; i++) R(i, j) = m[j * 4 + i];
        Eigen::Matrix<float, 3, 1> x(v[0], v[1], v[2]);
        Eigen::Matrix<float, 3, 1> a = M.block<3, 3>(0, 0) * x, b = R * x;
        for (int i = 0; i < 3; i++) { out[3 + i] = a(i); out[6 + i] = b(i); }
    }
}
"""


def _product_lib(tmp_path, fn, eigen_dir):
    src = tmp_path / f"{fn}.cpp"
    src.write_text(_PRODUCT_SRC % {"fn": fn})
    out = tmp_path / f"lib{fn}.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                    "-I" + os.path.join(ROOT, "densesurfelmapping_amd", "csrc"), "-I" + os.path.dirname(eigen_dir), str(src), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    lib.products.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def _operands(n=200_000):
    """random and hostile 3x3 (in a 4x4) and 3-vector operands"""
    rng = np.random.default_rng(33)
    m = rng.standard_normal((n, 16)).astype(np.float32)
    v = rng.standard_normal((n, 3)).astype(np.float32)
    q = n // 8
    # cancellation: a1*b1 ~ -a2*b2, large against a0*b0 -- the two trees round differently
    m[:q, 4 + 0] = np.float32(1e4)
    m[:q, 8 + 0] = np.float32(-1e4) * (1 + rng.uniform(-1e-6, 1e-6, q)).astype(np.float32)
    v[:q, 1] = v[:q, 2]
    # subnormals and values that underflow into them
    s = slice(q, 2 * q)
    m[s] *= np.float32(1e-38)
    v[s, 0] = np.float32(1e-41)
    # +-inf, NaN and signed zeros scattered through the operands
    s = slice(2 * q, 3 * q)
    pick = rng.random(m[s].shape)
    m[s] = np.where(pick < 0.03, np.float32(np.inf), np.where(pick < 0.06, np.float32(-np.inf),
                    np.where(pick < 0.09, np.float32(np.nan), np.where(pick < 0.15, np.float32(-0.0), m[s]))))
    pick = rng.random(v[s].shape)
    v[s] = np.where(pick < 0.05, np.float32(np.inf), np.where(pick < 0.1, np.float32(np.nan), np.where(pick < 0.2, np.float32(-0.0), v[s])))
    # near the top of the range: partial sums that overflow in one order only
    s = slice(3 * q, 4 * q)
    m[s] *= np.float32(1e19)
    v[s] *= np.float32(1e19)
    return np.ascontiguousarray(m), np.ascontiguousarray(v)


def _same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def test_xform_dir_e33_is_the_standin_product(tmp_path):
    """xform_dir_e33 == the stand-in's two 3x3 * 3x1 products bit for bit (NaN == NaN); xform_dir == the project's shim's;
    and the two orders differ on these operands."""
    m, v = _operands()
    n = len(m)
    res = {}
    for fn, eigen in (("xform_dir_e33", STANDIN), ("xform_dir", SHIM)):
        out = np.zeros((n, 9), np.float32)
        _product_lib(tmp_path, fn, eigen).products(m.ctypes.data, v.ctypes.data, out.ctypes.data, n)
        for k in (3, 6):
            ok = _same_bits(out[:, :3], out[:, k:k + 3])
            assert ok.all(), f"{fn} vs the shim's product ({k}): {int((~ok).sum())} differ, first rows {np.argwhere(~ok)[:3].tolist()}"
        res[fn] = out[:, :3]
    differ = ~_same_bits(res["xform_dir_e33"], res["xform_dir"])
    assert differ[: n // 8].sum() > 1000 and differ.sum() > 10_000, int(differ.sum())


def _surfels(a):
    from densesurfelmapping_amd import api
    return np.asarray(a).astype(api.SURFEL_DTYPE)


def test_every_fixture_differs_from_the_eigen32_order(oracle_built):
    """The C restatement (oracle/dsm_oracle.c: Eigen 3.2's order, the project's default) on the fixtures' own inputs: the same
    labels and seed geometry, a different map in every fixture.  A fixture the product order does not move would show
    nothing about the flag."""
    import eigen33_cases as E
    from densesurfelmapping_amd import api, synth
    from oracle import bindings as ob
    gold = _gold()
    assert [c["name"] for c in gold["sequences"]] == [c["name"] for c in E.SEQUENCES]
    for case, g in zip(E.SEQUENCES, gold["sequences"]):
        assert g["surfels_changed"] > 0 and g["frames_changed"] > 0, case["name"]
        orc = ob.PortOracle(getattr(synth, case["camera"]))
        lo = np.zeros(0, ob.SURFEL_DTYPE)
        for (t, img, dep, pose, ref), want in zip(E.sequence(case, synth), g["per_frame"]):
            lo, k = orc.fuse_map(ref, img, dep, pose, lo)
            rec = E.frame_record(k, _surfels(lo), orc.labels(), orc.seeds().astype(api.SEED_DTYPE))
            assert rec["labels_sha256"] == want["labels_sha256"], (case["name"], t)  # the superpixels do not see the map
        assert E.final_map_differences(_surfels(lo), g, GOLDEN) != [], f"{case['name']}: the Eigen 3.2 order reproduces the Eigen >= 3.3 fixture"
    assert [e["camera"] for e in gold["edge_cases"]] == E.EDGE_CAMERAS
    from test_gpu_parity import edge_cases
    for camera, g in zip(E.EDGE_CAMERAS, gold["edge_cases"]):
        cam = getattr(synth, camera)
        finals = np.load(os.path.join(GOLDEN, g["final_maps"]))
        moved = 0
        for name, (img, dep) in edge_cases(cam).items():
            orc = ob.PortOracle(cam)
            lo = np.zeros(0, ob.SURFEL_DTYPE)
            for ridx in (0, 1):
                lo, _ = orc.fuse_map(ridx, img, dep, E.EDGE_POSES[ridx], lo)
            moved += E.rows_differing(_surfels(lo), finals[name])
        assert moved > 0 and g["surfels_changed"] > 0, camera
    node = gold["node"]
    assert node["name"] == E.NODE_SCENARIO and node["records_changed"]["local"] > 0 and node["files_changed"]["ply"]


_FACADE_SRC = r"""
#include "dsm_fusion_functions.hpp"
#include "dsm_surfel_map.hpp"
static_assert(dsm::eigen_products_flag(3, 2) == 0u, "Eigen 3.2");
static_assert(dsm::eigen_products_flag(3, 3) == DSM_FLAG_EIGEN33_PRODUCTS, "Eigen 3.3");
static_assert(dsm::eigen_products_flag(3, 4) == DSM_FLAG_EIGEN33_PRODUCTS, "Eigen 3.4");
static_assert(dsm::eigen_products_flag(4, 0) == DSM_FLAG_EIGEN33_PRODUCTS, "Eigen 4");
static_assert(dsm::kDefaultEngineFlags == EXPECT, "default engine flags");
int main() {
    dsm::SurfelMap::Params p;
    return p.engine_flags == EXPECT ? 0 : 1;
}
"""


@pytest.mark.parametrize("match,version,expect", [
    (False, None, 0), (False, (3, 2), 0), (False, (3, 4), 0),  # without DSM_MATCH_CALLER_EIGEN: as before, whatever Eigen
    (True, (3, 2), 0), (True, (3, 3), 8), (True, (3, 4), 8),
    (True, None, None),  # asked to match an Eigen it cannot see: refused at compile time
])
def test_facade_picks_the_flag(tmp_path, match, version, expect):
    src = tmp_path / "facade.cpp"
    body = _FACADE_SRC
    if version:  # what <Eigen/Core> defines (Eigen/src/Core/util/Macros.h), before the dsm headers
        body = "#define EIGEN_WORLD_VERSION %d\n#define EIGEN_MAJOR_VERSION %d\n" % version + body
    src.write_text(body)
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)]
    if match:
        cmd.insert(1, "-DDSM_MATCH_CALLER_EIGEN")
    cmd.insert(1, "-DEXPECT=%du" % (expect or 0))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if expect is None:
        assert r.returncode != 0 and "DSM_MATCH_CALLER_EIGEN" in r.stderr, r.stderr
    else:
        assert r.returncode == 0, r.stderr
