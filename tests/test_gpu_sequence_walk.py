"""The one walk of the surfel sequence (csrc/dsm_k_sequence.h) through all four products that run it -- dsm_cloud_compose,
dsm_mesh_compose, dsm_render_compose, dsm_grid_compose -- over the same cases (tests/sequence_cases.py): the map sizes about the
wave, the workgroup and the tile; pass patterns that empty a wave or a tile; run lists of total length 0, 1, 63, 64, 65 in front
of the map part; a capacity that cuts inside a chunk.  Every output bit for bit against numpy (the cloud) or the product's
brute-force host checker; in the render and the grid every member of the sequence has a pixel / a voxel of its own
(tests/test_cpu_sequence_cases.py proves that of the inputs), so the index plane pins every sequence number."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import mesh_cases as mc
import render_cases as rc
import sequence_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 12345.0
CASES = sc.cases()


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    assert api_mod.CLOUD_TILE == sc.T
    return api_mod


def _engine_with_store(api, place):
    """an engine whose store holds sequence_cases' store records, in their order; returns (engine, those records)"""
    ff = api.FusionFunctions()
    ff.initialize(64, 32, 57.25, 55.5, 31.3, 15.7, 30.0, 0.3, surfel_capacity=1 << 13, frame_slots=2)
    store = sc.store_records(api.SURFEL_DTYPE, place)
    ff.map_upload(store)
    assert ff.store_deactivate(0) == (0, sc.STORE_N)
    held, _ = ff.store_download(0, sc.STORE_N)
    assert held.tobytes() == store.tobytes()  # (the inputs are as the expected values below take them to be)
    return ff, store


def _xyzi(s):
    return np.stack([s["px"], s["py"], s["pz"], s["color"]], axis=1).astype(np.float32).reshape(-1, 4)


def _cloud_expected(store, m, segs):
    return np.concatenate([_xyzi(sc.passing(m))] + [_xyzi(store[b:b + c]) for b, c in segs])  # the map part FIRST


def test_cloud(api):
    ff, store = _engine_with_store(api, sc.render_placed)
    for name, ut, segs in CASES:
        m = sc.render_placed(api.SURFEL_DTYPE, ut)
        ff.map_upload(m)
        mc.same_bits(np.asarray(ff.cloud_compose(sc.SELECT, segs), np.float32).reshape(-1, 4), _cloud_expected(store, m, segs), name)
    ff.close()


def test_mesh(api):
    ff, store = _engine_with_store(api, sc.render_placed)
    for name, ut, segs in CASES:
        m = sc.render_placed(api.SURFEL_DTYPE, ut)
        ff.map_upload(m)
        seq = sc.sequence(store, m, segs)
        for layout in (mc.REF6, mc.XYZ_RGBA8):
            mc.same_vertices(ff.mesh_compose(sc.SELECT, segs, layout), mc.host_vertices(seq, layout), layout, (name, layout))
    ff.close()


def test_render(api):
    ff, store = _engine_with_store(api, sc.render_placed)
    for name, ut, segs in CASES:
        m = sc.render_placed(api.SURFEL_DTYPE, ut)
        ff.map_upload(m)
        seq = sc.sequence(store, m, segs)
        got = ff.render(sc.SELECT, segs, sc.CAM, rc.IDENTITY)
        assert got["n_surfels"] == len(seq), name
        rc.same_planes(got, sc.expected("render", seq), name)
    ff.close()


def test_grid(api):
    ff, store = _engine_with_store(api, sc.grid_placed)
    spec = api.grid_spec(sc.GRID.origin[:], sc.GRID.voxel, gc.dims(sc.GRID), 0)
    for name, ut, segs in CASES:
        m = sc.grid_placed(api.SURFEL_DTYPE, ut)
        ff.map_upload(m)
        seq = sc.sequence(store, m, segs)
        got = ff.grid(sc.SELECT, segs, spec, 0, planes=("occupied", "inflated", "index", "cells"))
        exp = sc.expected("grid", seq)
        assert (got["n_surfels"], got["n_cells"]) == (len(seq), len(exp["cells"])), name
        gc.same_grids(got, exp, name)
    ff.close()


def _capped(api, call, words, cap, need):
    """call(dst, cap, n) into a guarded device buffer of `cap` records: DSM_E_CAPACITY, the count, nothing at or beyond cap"""
    import torch
    dev = torch.full((cap + 64, words), GUARD, dtype=torch.float32, device="cuda")
    n = C.c_int32(-1)
    assert call(C.c_void_p(dev.data_ptr()), cap, C.byref(n)) == api.DSM_E_CAPACITY and n.value == need
    d = dev.cpu().numpy()
    assert (d[cap:] == GUARD).all()
    return d[:cap]


@pytest.mark.parametrize("pattern", ["all pass", "alternating"])
def test_cap_inside_a_chunk(api, pattern):
    """the caller's capacity ends between two passing records of one 64-record chunk: in the first tile, in a later tile's second
    wave, and inside the runs"""
    ff, store = _engine_with_store(api, sc.render_placed)
    m = sc.render_placed(api.SURFEL_DTYPE, sc.PATTERNS[pattern])
    ff.map_upload(m)
    segs, n_map, n_run = sc.FRONT, len(sc.passing(m)), sc.run_total(sc.FRONT)
    per_chunk = 64 if pattern == "all pass" else 32
    inside = (per_chunk + per_chunk // 2 + 3, (sc.T + 256) // 64 * per_chunk + per_chunk + 7)  # map records below the cap
    b = np.array([s[0] for s in segs], np.int32)
    c = np.array([s[1] for s in segs], np.int32)
    lib = ff._lib
    exp = _cloud_expected(store, m, segs)  # the map part first: a cap inside it, then one inside the runs
    for cap in inside + (n_map + 30,):
        got = _capped(api, lambda dst, cap, n: lib.dsm_cloud_compose(ff._h, sc.SELECT, len(segs), b.ctypes.data, c.ctypes.data, dst, 1, cap, n), 4, cap,
                      len(exp))
        mc.same_bits(got, exp[:cap], ("cloud", cap))
    seq = sc.sequence(store, m, segs)       # the runs first
    for layout in (mc.REF6, mc.XYZ_RGBA8):
        exp = mc.host_vertices(seq, layout)
        for cap in (30,) + tuple(n_run + k for k in inside):
            got = _capped(api, lambda dst, cap, n: lib.dsm_mesh_compose(ff._h, sc.SELECT, len(segs), b.ctypes.data, c.ctypes.data, layout, dst, 1, cap, n),
                          mc.FLOATS[layout], cap, len(exp))
            mc.same_vertices(got, exp[:cap], layout, ("mesh", layout, cap))
    ff.close()
