"""Connected components on the GPU (dsm_grid_components, dsm_surfel_map_frontier_clusters*, msglog --save-frontier-clusters): every
label plane and every table equal, byte for byte, to the host checker of tests/components_host.cpp (a flood fill in ascending index
order, pinned to a Python restatement and to a second form by tests/test_cpu_components.py), on the case list of
tests/components_cases.py.  Destinations sit in poisoned device buffers with guard bytes behind them."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import components_cases as cc
import grid_cases as gc

ROOT = cc.ROOT
pytestmark = pytest.mark.gpu

GUARD = 0x4d   # the byte a poisoned destination holds
N_GUARD = 256  # guard bytes behind every device buffer
CAM = (64, 48, 60.0, 60.0, 32.0, 24.0)


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


@pytest.fixture(scope="module")
def ff(api):
    f = api.FusionFunctions()
    f.initialize(*CAM, 30.0, 0.3, surfel_capacity=1 << 12, frame_slots=2)
    yield f
    f.close()


def _buf(n_bytes, init=None):
    """a device buffer of n_bytes with guard bytes behind it: poisoned, or holding `init`"""
    import torch
    t = torch.full((n_bytes + N_GUARD,), GUARD, dtype=torch.uint8, device="cuda")
    if init is not None:
        t[:n_bytes] = torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).ravel()).cuda()
    return t


def _read(t, shape, dtype, what=""):
    a = t.cpu().numpy()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert (a[n:] == GUARD).all(), (what, "guard bytes written")
    return a[:n].view(dtype).reshape(shape).copy()


def _untouched(t, what=""):
    assert (t.cpu().numpy() == GUARD).all(), (what, "written")


def _run(api, ff, bits, nx, conn, min_count=1, tags=None, label=True, cap=None, what=""):
    """dsm_grid_components of a host bit set into guarded device buffers.  cap None: no table.  Returns {"n", "n_all", "label",
    "table" (the first min(n, cap) entries), "rest" (the bytes of the table buffer behind them), "code"}"""
    nz, ny, wx = bits.shape
    n_vox = nz * ny * nx
    src = _buf(bits.size * 4, bits)
    d_tag = None if tags is None else _buf(n_vox * 4, np.ascontiguousarray(tags, np.int32))
    d_label = _buf(n_vox * 4) if label else None
    d_table = None if cap is None else _buf(max(cap, 0) * 64)
    out = {"code": 0}
    try:
        out["n"], out["n_all"] = ff.grid_components((nx, ny, nz), src.data_ptr(), conn, min_count, None if d_tag is None else d_tag.data_ptr(),
                                                    None if d_label is None else d_label.data_ptr(), None if d_table is None else d_table.data_ptr(),
                                                    0 if cap is None else cap)
    except api.DsmError as e:
        if e.code != api.DSM_E_CAPACITY:
            raise
        out["code"], out["n"], out["n_all"] = e.code, e.n_components, e.n_all
    assert np.array_equal(_read(src, bits.shape, np.uint32, what), bits), (what, "the source is changed")
    if label:
        out["label"] = _read(d_label, (nz, ny, nx), np.int32, what)
    if cap is not None:
        raw = _read(d_table, (max(cap, 0) * 64,), np.uint8, what)
        k = min(out["n"], cap)
        out["table"], out["rest"] = raw[:k * 64].view(cc.COMPONENT).copy(), raw[k * 64:]
    return out


def _same(got, exp, what, cap=None):
    assert (got["n"], got["n_all"]) == (exp["n"], exp["n_all"]), (what, got["n"], got["n_all"], exp["n"], exp["n_all"])
    if "label" in got:
        bad = np.argwhere(got["label"] != exp["label"])
        assert bad.size == 0, (what, "label", len(bad), tuple(bad[0]), got["label"][tuple(bad[0])], exp["label"][tuple(bad[0])])
    if "table" in got:
        k = exp["n"] if cap is None else min(cap, exp["n"])
        assert len(got["table"]) == k, (what, len(got["table"]), k)
        if got["table"].tobytes() != exp["table"][:k].tobytes():
            j = next(i for i in range(k) if got["table"][i].tobytes() != exp["table"][i].tobytes())
            raise AssertionError((what, "table entry", j, got["table"][j], exp["table"][j]))
        assert (got["rest"] == GUARD).all(), (what, "written behind the entries")


def _case(api, ff, name, conn, min_count=1, dirty=False):
    c = cc.case(name)
    vox = c.vox()
    nx = vox.shape[2]
    bits = gc.pack(vox)
    if dirty:
        bits = np.array(bits)
        bits[..., -1] |= gc.pad_mask(nx)
    exp = cc.expected(name, conn, min_count)
    got = _run(api, ff, bits, nx, conn, min_count, cap=exp["n"] if c.table else None, what=(name, conn, min_count))
    _same(got, exp, (name, conn, min_count))
    return got, exp


# ------------------------------------------------------------------ 1. seams and diagonals
@pytest.mark.parametrize("kind", ("face", "edge", "corner"))
def test_pairs_across_word_wave_and_tile_seams(api, ff, kind):
    n_pairs = len(cc.seam_pairs(kind))
    for conn in (cc.FACES, cc.ALL):
        got, _ = _case(api, ff, "seam %s pairs" % kind, conn, dirty=True)
        assert got["n_all"] == (n_pairs if kind == "face" or conn == cc.ALL else 2 * n_pairs)


# ------------------------------------------------------------------ 2. percolation
@pytest.mark.parametrize("conn", (cc.FACES, cc.ALL))
def test_percolation(api, ff, conn):
    for d in cc.PERCOLATION[conn]:
        got, exp = _case(api, ff, "percolation %d at %g" % (conn, d), conn, dirty=True)
        print("percolation", conn, d, "components", got["n_all"], "largest", int(exp["table"]["count"].max()))


# ------------------------------------------------------------------ 3. long chains
@pytest.mark.parametrize("name", ("serpentine", "serpentine mirrored", "u shape"))
def test_long_chains(api, ff, name):
    for conn in (cc.FACES, cc.ALL):
        got, _ = _case(api, ff, name, conn)
        assert got["n_all"] == 1 and got["table"]["root"][0] == np.flatnonzero(cc.case(name).vox().ravel())[0]


# ------------------------------------------------------------------ 4. extremes
def test_extremes(api, ff):
    for conn in (cc.FACES, cc.ALL):
        vox = cc.case("empty").vox()
        got = _run(api, ff, gc.pack(vox), vox.shape[2], conn, cap=4, what="empty")
        assert (got["n"], got["n_all"]) == (0, 0) and (got["label"] == -1).all() and (got["rest"] == GUARD).all()
        _case(api, ff, "all set 33x5x3", conn, dirty=True)
        _case(api, ff, "one voxel", conn, dirty=True)
        _case(api, ff, "nx 1", conn, dirty=True)
        got, _ = _case(api, ff, "checkerboard 34x6x4", conn, dirty=True)
        assert got["n_all"] == (34 * 6 * 4 // 2 if conn == cc.FACES else 1)
    # pad bits alone make nothing
    bits = np.zeros((3, 5, 2), np.uint32)
    bits[..., -1] = gc.pad_mask(33)
    got = _run(api, ff, bits, 33, cc.ALL, cap=2, what="pads only")
    assert (got["n"], got["n_all"]) == (0, 0) and (got["label"] == -1).all()


# ------------------------------------------------------------------ 5. past the launch caps and past 32 bits
def test_one_component_with_sums_past_32_bits(api, ff):
    got, exp = _case(api, ff, "all set 2x2000x2000", cc.FACES)
    assert got["n_all"] == 1 and int(got["table"]["sum"][0][1]) == 2 * sum(range(2000)) * 2000 > 2 ** 32


def test_more_roots_than_one_trip_of_the_count_and_scan(api, ff):
    name = "checkerboard 2x1500x1500"
    vox = cc.case(name).vox()
    exp = cc.expected(name, cc.FACES, 2)
    got = _run(api, ff, gc.pack(vox), 2, cc.FACES, 2, what=name)  # table NULL
    _same(got, exp, name)
    assert (got["n"], got["n_all"]) == (0, 2_250_000)


# ------------------------------------------------------------------ 6. filter and capacity
def test_filter_and_capacity(api, ff):
    name = "sizes 1 to 6"
    vox = cc.case(name).vox()
    bits, nx = gc.pack(vox), vox.shape[2]
    for conn in (cc.FACES, cc.ALL):
        for mc, kept in ((1, 6), (3, 4), (6, 1), (7, 0)):
            got, exp = _case(api, ff, name, conn, mc)
            assert got["n"] == kept and np.array_equal(got["label"], cc.expected(name, conn, 1)["label"])  # the labels are never filtered
            assert list(got["table"]["root"]) == sorted(got["table"]["root"]) and (got["table"]["count"] >= mc).all()
        exp = cc.expected(name, conn, 3)
        for cap in (exp["n"] - 1, 1, 0):
            got = _run(api, ff, bits, nx, conn, 3, cap=cap, what=(name, "cap", cap))
            assert got["code"] == api.DSM_E_CAPACITY and got["n"] == exp["n"]
            _same(got, exp, (name, "cap", cap), cap=cap)  # the label complete, the entries that fit complete, nothing behind them
        got = _run(api, ff, bits, nx, conn, 7, cap=0, what=(name, "cap 0, none kept"))
        assert got["code"] == 0 and got["n"] == 0
        got = _run(api, ff, bits, nx, conn, 3, label=False, cap=exp["n"], what=(name, "table only"))
        _same(got, exp, (name, "table only"))


# ------------------------------------------------------------------ 7. tags
def test_tags(api, ff):
    rng = np.random.default_rng(12)
    vox = cc.random_set((70, 9, 5), 0.2, 77)
    tags = rng.integers(-2**31, 2**31, vox.shape, dtype=np.int64).astype(np.int32)
    for conn in (cc.FACES, cc.ALL):
        exp = cc.host_components(gc.pack(vox), 70, conn, 2, tags=tags)
        got = _run(api, ff, gc.pack(vox), 70, conn, 2, tags=tags, cap=exp["n"], what="tags")
        _same(got, exp, ("tags", conn))
        assert np.array_equal(got["table"]["tag"], tags.ravel()[got["table"]["root"]]) and len(got["table"]) > 5
        plain = _run(api, ff, gc.pack(vox), 70, conn, 2, cap=exp["n"], what="no tags")
        assert (plain["table"]["tag"] == 0).all() and (plain["table"]["reserved"] == 0).all()


# ------------------------------------------------------------------ 8. arguments
def test_refusals_touch_nothing(api, ff):
    import torch
    g = (33, 5, 3)
    nx, ny, nz = g
    bits = gc.pack(cc.random_set(g, 0.3, 1))
    n_vox, n_words = nx * ny * nz, bits.size
    src, tag, label, table = _buf(n_words * 4, bits), _buf(n_vox * 4, np.zeros(n_vox, np.int32)), _buf(n_vox * 4), _buf(8 * 64)
    lib = ff._lib
    n, n_all = C.c_int32(-7), C.c_int32(-7)

    def call(dims=g, conn=26, mc=1, s=src.data_ptr(), t=None, lab=label.data_ptr(), tab=table.data_ptr(), cap=8, h=ff._h, planes=True, count=True):
        st = api._ComponentPlanes(lab, tab, cap)
        return lib.dsm_grid_components(h, dims[0], dims[1], dims[2], conn, mc, s, t, C.byref(st) if planes else None, C.byref(n) if count else None,
                                       C.byref(n_all))

    big = torch.empty(1, dtype=torch.uint8, device="cuda").data_ptr() & ~7  # (never dereferenced: the call is refused first)
    refused = {
        "null handle": dict(h=None), "null source": dict(s=None), "null planes": dict(planes=False), "null n_components": dict(count=False),
        "nx 0": dict(dims=(0, 5, 3)), "ny -1": dict(dims=(33, -1, 3)), "nz 0": dict(dims=(33, 5, 0)),
        "more than 2^26 voxels": dict(dims=(4096, 4096, 5), s=big, lab=None, tab=big + 4096, cap=0),
        "connectivity 18": dict(conn=18), "connectivity 0": dict(conn=0), "min_count 0": dict(mc=0), "min_count -3": dict(mc=-3),
        "both outputs null": dict(lab=None, tab=None), "table_cap -1": dict(cap=-1),
        "label and table the same": dict(tab=label.data_ptr()), "table inside label": dict(tab=label.data_ptr() + 64),
        "label over the source": dict(lab=src.data_ptr()), "table over the source": dict(tab=src.data_ptr() + 8),
        "label over the tags": dict(t=tag.data_ptr(), lab=tag.data_ptr() + 16), "table over the tags": dict(t=tag.data_ptr(), tab=tag.data_ptr() + 64),
        "source not aligned": dict(s=src.data_ptr() + 2), "tags not aligned": dict(t=tag.data_ptr() + 1), "label not aligned": dict(lab=label.data_ptr() + 2),
        "table not 8-byte aligned": dict(tab=table.data_ptr() + 4),
    }
    for what, kw in refused.items():
        assert call(**kw) == api.DSM_E_INVALID, what
        assert (n.value, n_all.value) == (-7, -7), what
        _untouched(label, what)
        _untouched(table, what)
        assert np.array_equal(_read(src, bits.shape, np.uint32), bits)
    assert call() == 0 and n.value == cc.host_components(bits, nx, 26)["n"]  # and the same call without a fault goes through


# ------------------------------------------------------------------ 9. repeatability on shared scratch
def test_repeatable_and_interleaved_with_the_other_grid_calls(api, ff):
    import torch
    g = cc.SEAM_GRID
    nx, ny, nz = g
    runs = {}
    for conn in (cc.FACES, cc.ALL):
        name = "percolation %d at %g" % (conn, cc.PERCOLATION[conn][1])
        bits, exp = gc.pack(cc.case(name).vox()), cc.expected(name, conn)
        first = _run(api, ff, bits, nx, conn, cap=exp["n"], what=name)
        _same(first, exp, name)
        runs[conn] = (name, bits, exp, first)
    n_vox, n_words = nx * ny * nz, runs[cc.FACES][1].size
    src = _buf(n_words * 4, runs[cc.FACES][1])
    other = _buf(n_words * 4, runs[cc.ALL][1])
    for k in range(2):
        for conn in (cc.ALL, cc.FACES):
            name, bits, exp, first = runs[conn]
            # the other products of this handle in between: their scratch is the handle's too
            dist = torch.empty(n_vox, dtype=torch.int16, device="cuda")
            ff.grid_distance(g, 5 + k, 0.1, src.data_ptr(), {"dist2": dist.data_ptr()})
            planes = {"frontier": _buf(n_words * 4), "cells": _buf(64 * 4)}
            try:
                ff.grid_classify(g, src.data_ptr(), other.data_ptr(), {p: t.data_ptr() for p, t in planes.items()}, cells_cap=64)
            except api.DsmError as e:
                assert e.code == api.DSM_E_CAPACITY
            infl = _buf(n_words * 4)
            ff.grid_inflate(g, 1 + k, src.data_ptr(), infl.data_ptr())
            again = _run(api, ff, bits, nx, conn, cap=exp["n"], what=(name, "again", k))
            assert again["label"].tobytes() == first["label"].tobytes() and again["table"].tobytes() == first["table"].tobytes(), (name, k)
            assert (again["n"], again["n_all"]) == (first["n"], first["n_all"])


def test_host_convenience(api, ff):
    vox = cc.case("sizes 1 to 6").vox()
    exp = cc.expected("sizes 1 to 6", cc.ALL, 3)
    table, n_all, labels = ff.grid_components_host(gc.pack(vox), vox.shape[2], cc.ALL, 3)
    assert table.dtype == api.COMPONENT_DTYPE and table.tobytes() == exp["table"].tobytes() and n_all == 6 and np.array_equal(labels, exp["label"])


# ------------------------------------------------------------------ 10. the node and msglog
NODE_VOXEL, NODE_DIMS = 0.5, (32, 160, 16)  # around the origin, where the first camera sits; it drives along +y, z is up
NODE_CARVE = dict(near_dist=0.5, far_dist=25.0, margin=0.9)
NODE_FRAMES = 14


def test_node_frontier_clusters(api, tmp_path):
    from densesurfelmapping_amd import msglog, surfel_map, synth
    import node_state
    case = node_state.SCENARIOS[0]
    (cam, scene), dfp = node_state.camera_and_scene(case, synth), case["drift_free_poses"]
    events = list(synth.node_messages(cam, scene, NODE_FRAMES, **case["kw"]))
    log = str(tmp_path / "node.dsmlog")
    msglog.write_log(log, cam, dfp, iter(events))
    # The camera travels at z = 0, which a grid centred on the origin has as a lattice plane; it sees ground and walls, nothing above its
    # horizon, so the voxels whose centres lie above it stay unknown.  With the lattice 0.1 m higher, the voxel that holds the camera has
    # its centre 0.15 m below it: seen through by the frames before.
    around = api.grid_spec_around((0.0, 0.0, 0.0), NODE_VOXEL, NODE_DIMS)
    spec = api.grid_spec((around.origin[0], around.origin[1], around.origin[2] + 0.1), NODE_VOXEL, NODE_DIMS, 0)
    nx, ny, nz = NODE_DIMS
    n_vox, n_words = nx * ny * nz, nz * ny * ((nx + 31) // 32)
    node = surfel_map.SurfelMap(cam, drift_free_poses=dfp)
    with pytest.raises(api.DsmError) as e:  # DSM_E_STATE before set_free_space ...
        node.frontier_clusters()
    assert e.value.code == api.DSM_E_STATE
    node.set_free_space(spec, NODE_CARVE)
    with pytest.raises(api.DsmError) as e:  # ... and before the first fuse
        node.frontier_clusters()
    assert e.value.code == api.DSM_E_STATE
    for ev in events:
        node.feed(ev)
    assert node.frames_fused > 5
    before = (node_state.digest(node_state.snapshot(node)), node.free_space()[0].tobytes(), node.free_space()[1])
    # the planes dsm_surfel_map_space_device returns for this state: what the clusters are defined on
    bufs = {"known_free": _buf(n_words * 4), "frontier": _buf(n_words * 4)}
    _, n_frontier = node.space("all", dst_ptrs={k: t.data_ptr() for k, t in bufs.items()})
    frontier, known_free = (_read(bufs[k], (nz, ny, (nx + 31) // 32), np.uint32) for k in ("frontier", "known_free"))
    assert n_frontier == int(gc.unpack(frontier, nx).sum()) > 50
    regions = cc.host_components(known_free, nx, cc.FACES)["label"]
    pose = node.last_pose()
    origin = pose[:3, 3].copy()
    at = cc.from_voxel(origin, spec.origin[:], spec.voxel)
    print("from", origin, "in voxel", at, "known-free column", regions[:, at[1], at[0]].tolist())
    occupied = np.argwhere(gc.unpack(node.grid("all", spec=spec, planes=("occupied",))["occupied"], nx))[0][::-1]
    on_occupied = [spec.origin[a] + (float(occupied[a]) + 0.5) * spec.voxel for a in range(3)]
    for conn in (cc.FACES, cc.ALL):
        for mc in (1, 3):
            plain = cc.host_components(frontier, nx, conn, mc)
            got = node.frontier_clusters("all", conn, mc, labels=True)
            assert got["table"].tobytes() == plain["table"].tobytes() and got["n_all"] == plain["n_all"] and got["from_root"] == -1, (conn, mc)
            assert np.array_equal(got["labels"], plain["label"])
            assert (got["table"]["tag"] == 0).all() and len(got["table"]) == plain["n"] > 0
            # reachability: the tag is the known-free region of the cluster's root voxel
            exp = cc.host_components(frontier, nx, conn, mc, tags=regions)
            got = node.frontier_clusters("all", conn, mc, origin=origin, labels=True)
            want_root = int(regions[at[2], at[1], at[0]])
            assert got["table"].tobytes() == exp["table"].tobytes() and np.array_equal(got["labels"], exp["label"]), (conn, mc)
            assert got["from_root"] == want_root >= 0 and (got["table"]["tag"] == want_root).any() and (got["table"]["tag"] >= 0).all(), (conn, mc)
            # device destinations, guarded; a table one entry short
            d_table, d_label = _buf(exp["n"] * 64), _buf(n_vox * 4)
            assert node.frontier_clusters("all", conn, mc, origin=origin, dst_ptrs={"table": d_table.data_ptr(), "label": d_label.data_ptr()},
                                          table_cap=exp["n"]) == (exp["n"], exp["n_all"], want_root)
            assert _read(d_table, (exp["n"],), cc.COMPONENT).tobytes() == exp["table"].tobytes()
            assert np.array_equal(_read(d_label, (nz, ny, nx), np.int32), exp["label"])
            d_short = _buf((exp["n"] - 1) * 64)
            with pytest.raises(api.DsmError) as e:
                node.frontier_clusters("all", conn, mc, origin=origin, dst_ptrs={"table": d_short.data_ptr()}, table_cap=exp["n"] - 1)
            assert e.value.code == api.DSM_E_CAPACITY and e.value.n_clusters == exp["n"]
            assert _read(d_short, (exp["n"] - 1,), cc.COMPONENT).tobytes() == exp["table"][:-1].tobytes()
            with pytest.raises(api.DsmError) as e:
                node.frontier_clusters("all", conn, mc, table_cap=exp["n"] - 1)
            assert e.value.code == api.DSM_E_CAPACITY and e.value.table.tobytes() == plain["table"][:-1].tobytes()
    # from outside the grid, and on an occupied voxel
    assert node.frontier_clusters("all", origin=(1e4, 0.0, 0.0))["from_root"] == -1
    assert node.frontier_clusters("all", origin=on_occupied)["from_root"] == -1
    for bad in (dict(connectivity=18), dict(min_count=0), dict(kind="raw")):
        with pytest.raises(api.DsmError) as e:
            node.frontier_clusters(**bad)
        assert e.value.code == api.DSM_E_INVALID, bad
    q = surfel_map._FrontierQuery()
    node._lib.dsm_frontier_query_init(C.byref(q))
    q.struct_size -= 4
    table, n = np.zeros(4, cc.COMPONENT), C.c_int32(0)
    assert node._lib.dsm_surfel_map_frontier_clusters(node._h, 2, C.byref(q), table.ctypes.data, 4, None, C.byref(n), None, None) == api.DSM_E_INVALID
    # the clouds, the map and the accumulator are unchanged
    assert (node_state.digest(node_state.snapshot(node)), node.free_space()[0].tobytes(), node.free_space()[1]) == before
    node.close()
    # what msglog replays: the same log with the grid centred on the first pose
    node = surfel_map.SurfelMap(cam, drift_free_poses=dfp)
    node.set_free_space(api.grid_spec_around((0.0, 0.0, 0.0), NODE_VOXEL, NODE_DIMS), NODE_CARVE)
    for ev in events:
        node.feed(ev)
    want = node.frontier_clusters("all", 26, 2, origin=node.last_pose()[:3, 3])
    node.close()
    # msglog --save-frontier-clusters round-trips the table (a process of its own: that is what the command is)
    out = str(tmp_path / "clusters.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "densesurfelmapping_amd.msglog", log, "--save-frontier-clusters", out, "--cluster-min", "2", "--cluster-connect", "26",
                          "--grid-voxel", str(NODE_VOXEL), "--grid-dims"] + [str(d) for d in NODE_DIMS] + ["--carve-near", "0.5", "--carve-far", "25", "--carve-margin", "0.9"],
                         capture_output=True, text=True, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    saved = np.load(out)
    assert saved["table"].dtype == api.COMPONENT_DTYPE and saved["table"].tobytes() == want["table"].tobytes()
    assert int(saved["from_root"]) == want["from_root"] and int(saved["n_all"]) == want["n_all"] and saved["dims"].tolist() == list(NODE_DIMS)
    assert summary["frontier_clusters"] == len(want["table"]) and summary["frontier_clusters_all"] == want["n_all"]
