"""The hexagon mesh without a GPU: the corner function the HIP kernels call (surfel_hexagon of csrc/dsm_math.h, compiled for
the host by tests/mesh_host.cpp with -ffp-contract=off) against a numpy restatement of the reference's push_a_surfel
(surfel_fusion/src/surfel_map.cpp:1176-1216) -- bit for bit, NaN == NaN --, against the reference node's own PLY files
(the digests of tests/golden/node_golden.json), and the declarations, exports, index pattern and binary PLY layout."""
import ctypes as C
import json
import os
import re

import numpy as np

import mesh_cases as mc
import node_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dtype():
    from densesurfelmapping_amd import api
    return api.SURFEL_DTYPE


def test_corner_function_random_bit_patterns():
    rng = np.random.default_rng(17)
    for n in (1, 4097):
        s = mc.random_records(rng, n, _dtype())
        mc.same_bits(mc.host_vertices(s), mc.np_hexagon(s), ("random bits", n))
    s = mc.plausible_records(rng, 20000, _dtype())
    got = mc.host_vertices(s)
    assert np.isfinite(got).all()
    mc.same_bits(got, mc.np_hexagon(s), "plausible")


def test_corner_function_crafted_records():
    s, names = mc.crafted_records(_dtype())
    got, exp = mc.host_vertices(s), mc.np_hexagon(s)
    for i, name in enumerate(names):
        mc.same_bits(got[i:i + 1], exp[i:i + 1], name)
    v = got.reshape(len(s), 6, 6)
    # nx = ny = 0: squaredNorm 0, no normalise, x_dir = y_dir = (+-0, +-0, +-0): every corner is the position
    for i in (0, 1, 2, 4):
        assert (v[i, :, :3] == np.array([1.5, -2.25, 3.125], np.float32)).all(), names[i]
    # 1e-30 squared underflows to 0 as well
    assert (v[5, :, :3] == np.array([1.5, -2.25, 3.125], np.float32)).all(), names[5]
    # an overflowing squaredNorm divides by inf: x_dir = 0, again the position
    assert (v[7, :, :3] == np.array([1.5, -2.25, 3.125], np.float32)).all(), names[7]
    # inf size: inf - inf somewhere in every corner's sum, or inf itself
    assert not np.isfinite(v[10, :, :3]).all()
    # colours: (float)(int)color, INT_MIN for a NaN and outside int
    k0 = names.index("colour 0.0")
    want = [0, 255, -1, 300, mc.INT_MIN, mc.INT_MIN, mc.INT_MIN, 2147483520, mc.INT_MIN, mc.INT_MIN, 0, mc.INT_MIN, mc.INT_MIN]
    assert len(want) == len(mc.CRAFTED_COLORS)
    lib = mc.host_lib()
    for j, (c, w) in enumerate(zip(mc.CRAFTED_COLORS, want)):
        assert lib.mesh_host_color_int(C.c_float(c)) == w, (c, w)
        assert (v[k0 + j, :, 3:] == np.float32(w)).all(), (c, w)
    assert np.array_equal(mc.np_color_int(np.array(mc.CRAFTED_COLORS, np.float32)), np.array(want, np.int32))


def test_rgba8_layout_is_ref6_with_clamped_bytes():
    rng = np.random.default_rng(23)
    s = np.concatenate([mc.crafted_records(_dtype())[0], mc.random_records(rng, 3000, _dtype()), mc.plausible_records(rng, 3000, _dtype())])
    got = mc.host_vertices(s, mc.XYZ_RGBA8)
    mc.same_vertices(got, mc.ref6_to_rgba8(mc.host_vertices(s, mc.REF6)), mc.XYZ_RGBA8, "rgba8 vs ref6")
    rgba = got.reshape(-1, 4)[:, 3].view(np.uint32)
    assert ((rgba >> 24) == 255).all()
    k0 = mc.crafted_records(_dtype())[1].index("colour 0.0")
    want = [0, 255, 0, 255, 0, 0, 0, 255, 0, 0, 0, 0, 0]  # clamp((int)color): -1 -> 0, 300 -> 255, INT_MIN -> 0
    for j, w in enumerate(want):
        assert (rgba.reshape(-1, 6)[k0 + j] & 0xffffff == w * 0x010101).all(), (mc.CRAFTED_COLORS[j], w)


def test_ref6_printed_like_the_reference_is_the_reference_nodes_ply(tmp_path):
    """the goldens' final states through the corner function, printed as save_mesh prints `vertexs`, are the PLY files the
    reference node wrote (sha256 and size in node_golden.json)"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "node_golden.json")))
    checked = 0
    for case in gold["cases"]:
        if not case["final"]:
            continue
        fin = np.load(os.path.join(ROOT, "tests", "golden", case["final"]))
        local = fin["local"]
        # save_mesh's order: the attached surfels keyframe by keyframe (the snapshot's order), then the mature active ones
        s = np.concatenate([fin["attached"], local[local["update_times"] >= 5]])
        path = tmp_path / (case["name"] + ".ply")
        mc.print_ref6(path, mc.host_vertices(s))
        d = node_state.file_digest(str(path))
        assert d["bytes"] == case["files"]["ply"]["bytes"], case["name"]
        assert d["sha256"] == case["files"]["ply"]["sha256"], case["name"]
        checked += 1
    assert checked == len(node_state.SCENARIOS)


def test_declarations_and_exports():
    from densesurfelmapping_amd import api, build, surfel_map
    build.build_library()
    lib = C.CDLL(api.LIB_PATH)
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dsm_h = strip(open(os.path.join(ROOT, "include", "dsm.h")).read())
    node_h = strip(open(os.path.join(ROOT, "include", "dsm_surfel_map.h")).read())
    for name in ("dsm_mesh_compose", "dsm_mesh_indices"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", dsm_h), name
        assert name in api.ABI_SYMBOLS and hasattr(lib, name), name
    for name in ("dsm_surfel_map_get_mesh", "dsm_surfel_map_get_mesh_device", "dsm_surfel_map_save_mesh_binary"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", node_h), name
        assert name in surfel_map.ABI_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"DSM_MESH_VERTEX_REF6\s*=\s*0", dsm_h) and re.search(r"DSM_MESH_VERTEX_XYZ_RGBA8\s*=\s*1", dsm_h)
    assert (api.MESH_VERTEX_REF6, api.MESH_VERTEX_XYZ_RGBA8) == (0, 1)
    assert api.MESH_SURFEL_BYTES == {0: 144, 1: 96}
    assert re.search(r"#define\s+DSM_ABI_VERSION\s+4\b", dsm_h)  # additive: no bump
    for method in ("mesh_compose", "mesh_indices"):
        assert callable(getattr(api.FusionFunctions, method))
    for method in ("get_mesh", "save_mesh_binary"):
        assert callable(getattr(surfel_map.SurfelMap, method))
    hpp = open(os.path.join(ROOT, "include", "dsm_surfel_map.hpp")).read()
    assert "int get_mesh(" in hpp and "int save_mesh_binary(" in hpp
    # argument checks come before any device call
    lib.dsm_mesh_compose.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int32, C.c_void_p]
    lib.dsm_mesh_indices.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int]
    assert lib.dsm_mesh_compose(None, 1, 0, None, None, 0, None, 0, 0, None) == api.DSM_E_INVALID
    assert lib.dsm_mesh_indices(None, 0, None, 0) == api.DSM_E_INVALID
    lib.dsm_surfel_map_save_mesh_binary.argtypes = [C.c_void_p, C.c_char_p]
    assert lib.dsm_surfel_map_save_mesh_binary(None, b"x") == api.DSM_E_INVALID


def test_index_pattern(tmp_path):
    """the faces the binary writer (csrc/dsm_mesh_ply.h) emits are the reference's (p1 p2 p3) (p2 p4 p3) (p3 p4 p5) (p5 p4 p6)
    with p1..p6 = 6 i .. 6 i + 5 (:1270-1278) -- the pattern 6 i + {0,1,2, 1,3,2, 2,3,4, 4,3,5} of k_mesh_indices, which
    tests/test_gpu_mesh.py holds against the same table"""
    n = 5
    path = tmp_path / "faces.ply"
    v = np.zeros((n * 6, 4), np.float32)
    assert mc.host_lib().mesh_host_ply_binary(str(path).encode(), v.ctypes.data, n) == 0
    _, _, faces, _ = mc.read_ply_binary(str(path))
    want = []
    for i in range(n):
        p1, p2, p3, p4, p5, p6 = (6 * i + k for k in range(6))
        want += [[p1, p2, p3], [p2, p4, p3], [p3, p4, p5], [p5, p4, p6]]
    assert faces.tolist() == want
    assert mc.expect_faces(n).tolist() == want  # the table the GPU tests compare dsm_mesh_indices with


def test_binary_ply_writer_layout(tmp_path):
    """csrc/dsm_mesh_ply.h on a hand-made XYZ_RGBA8 buffer: header, 15-byte vertices, 13-byte faces"""
    for n in (0, 1, 3, (1 << 14) + 5):  # (past one block of the face writer; 6 n past one block of the vertex writer)
        v = np.zeros((n * 6, 4), np.float32)
        v[:, :3] = np.arange(n * 18, dtype=np.float32).reshape(-1, 3) * np.float32(0.5) - np.float32(7)
        b = (np.arange(n * 6, dtype=np.uint32) * 7) % 256
        v[:, 3] = (b | ((b ^ 1) << 8) | ((b ^ 2) << 16) | np.uint32(0xff000000)).astype(np.uint32).view(np.float32)
        if n:
            v[0, 0] = np.uint32(0x7fc12345).view(np.float32)  # a NaN payload passes through
        path = tmp_path / f"m{n}.ply"
        assert mc.host_lib().mesh_host_ply_binary(str(path).encode(), v.ctypes.data, n) == 0
        pos, col, faces, head = mc.read_ply_binary(str(path))
        assert head[:11] == ["ply", "format binary_little_endian 1.0", f"element vertex {n * 6}", "property float x", "property float y",
                             "property float z", "property uchar red", "property uchar green", "property uchar blue",
                             f"element face {n * 4}", "property list uchar int vertex_index"]
        assert head[11] == "end_header"
        assert np.array_equal(pos.view(np.uint32), v[:, :3].copy().view(np.uint32))
        assert np.array_equal(col, np.stack([b, b ^ 1, b ^ 2], axis=1).astype(np.uint8))
        assert np.array_equal(faces, mc.expect_faces(n))
    assert mc.host_lib().mesh_host_ply_binary(str(tmp_path / "no_such_dir" / "m.ply").encode(), None, 0) == -1
