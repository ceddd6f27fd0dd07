"""The hexagon mesh on the GPU (dsm_mesh_compose / dsm_mesh_indices, dsm_surfel_map_get_mesh* / dsm_surfel_map_save_mesh_binary):
every vertex buffer bit-identical (NaN == NaN) to the host build of the same corner function (tests/mesh_host.cpp), which
tests/test_cpu_mesh.py pins to the reference's push_a_surfel and to the reference node's PLY files."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_cases as mc
import node_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

LAYOUTS = (mc.REF6, mc.XYZ_RGBA8)
GUARD = 12345.0


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


def _engine(api, cap=1 << 15):
    ff = api.FusionFunctions()
    ff.initialize(64, 32, 57.25, 55.5, 31.3, 15.7, 30.0, 0.3, surfel_capacity=cap, frame_slots=2)
    return ff


def _records(rng, n, api, ut=None):
    """half arbitrary bit patterns, half ordinary finite records, interleaved at random"""
    a = mc.random_records(rng, n, api.SURFEL_DTYPE, ut)
    b = mc.plausible_records(rng, n, api.SURFEL_DTYPE, ut)
    pick = rng.random(n) < 0.5
    a[pick] = b[pick]
    if ut is not None:
        a["update_times"] = ut
    return a


def _keep(m, select):
    if select == 0:
        return m[:0]
    return m[m["update_times"] >= 5] if select == 1 else m[m["update_times"] != 0]


def _device_compose(ff, select, segs, layout, n_expect, slack=8):
    """compose into a torch buffer with guard records behind; returns the records written"""
    import torch
    words = mc.FLOATS[layout]
    dev = torch.full((n_expect + slack, words), GUARD, dtype=torch.float32, device="cuda")
    n = ff.mesh_compose(select, segs, layout, dst_ptr=dev.data_ptr(), cap=n_expect + slack)
    d = dev.cpu().numpy()
    assert n == n_expect
    assert (d[n:] == GUARD).all()
    return d[:n]


def _check_all(ff, m, what, selects=(1, 2)):
    for sel in selects:
        kept = _keep(m, sel)
        for layout in LAYOUTS:
            exp = mc.host_vertices(kept, layout)
            mc.same_vertices(ff.mesh_compose(sel, (), layout), exp, layout, (what, sel, layout, "host"))
            mc.same_vertices(_device_compose(ff, sel, (), layout, len(exp)), exp, layout, (what, sel, layout, "device"))


# ------------------------------------------------------------------ 1. the map part
def test_compose_edge_sizes(api):
    rng = np.random.default_rng(7)
    ff = _engine(api)
    T = api.CLOUD_TILE
    for n in (0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17):
        m = _records(rng, n, api)
        ff.map_upload(m)
        _check_all(ff, m, n)
    ff.close()


def test_compose_pass_patterns(api):
    rng = np.random.default_rng(9)
    ff = _engine(api)
    T = api.CLOUD_TILE
    n = 5 * T + 3
    last = np.zeros(n, np.int32)
    last[-1] = 5
    for name, ut in (("none pass", np.zeros(n, np.int32)), ("all pass", np.full(n, 7, np.int32)),
                     ("alternating", np.where(np.arange(n) % 2 == 0, 5, 4).astype(np.int32)),
                     ("every 64th", np.where(np.arange(n) % 64 == 63, 9, 0).astype(np.int32)),
                     ("last only", last)):
        m = _records(rng, n, api, ut)
        ff.map_upload(m)
        _check_all(ff, m, name)
    ff.close()


def test_compose_crafted_records(api):
    ff = _engine(api)
    m, _ = mc.crafted_records(api.SURFEL_DTYPE)
    ff.map_upload(m)
    _check_all(ff, m, "crafted", selects=(1,))
    ff.close()


def test_compose_destination_alignment(api):
    """a device destination that is only 4-byte aligned: the dword head and tail around the 16-byte body"""
    import torch
    rng = np.random.default_rng(21)
    ff = _engine(api)
    T = api.CLOUD_TILE
    m = _records(rng, 2 * T + 77, api)
    ff.map_upload(m)
    for layout in LAYOUTS:
        exp = mc.host_vertices(_keep(m, 1), layout)
        words = exp.size
        for shift in (1, 2, 3):
            dev = torch.full((words + 16,), GUARD, dtype=torch.float32, device="cuda")
            n = ff.mesh_compose(1, (), layout, dst_ptr=dev.data_ptr() + 4 * shift, cap=len(exp))
            d = dev.cpu().numpy()
            assert n == len(exp)
            assert (d[:shift] == GUARD).all() and (d[shift + words:] == GUARD).all()
            mc.same_vertices(d[shift:shift + words], exp, layout, ("shift", shift, layout))
    with pytest.raises(api.DsmError) as e:
        ff.mesh_compose(1, (), 0, dst_ptr=dev.data_ptr() + 2, cap=len(exp))
    assert e.value.code == api.DSM_E_INVALID
    n = C.c_int32(0)
    assert ff._lib.dsm_mesh_compose(ff._h, 1, 0, None, None, 2, C.c_void_p(dev.data_ptr()), 1, 8, C.byref(n)) == api.DSM_E_INVALID  # no such layout
    ff.close()


# ------------------------------------------------------------------ 2. store runs
def test_store_runs(api):
    import torch
    rng = np.random.default_rng(5)
    ff = _engine(api)
    m = _records(rng, 20000, api)
    m["last_update"] = rng.integers(0, 9, len(m))
    ff.map_upload(m)
    for key in (3, 0, 7, 5):
        ff.store_deactivate(key)
    store_n = ff.store_size()
    store, _ = ff.store_download(0, store_n)
    live = ff.map_download()
    assert store_n > 2000
    cases = [[], [(0, store_n)], [(5, 0), (0, 0)],                                   # empty list, everything, empty runs
             [(store_n - 1, 1), (0, 3), (100, 50), (7, 0), (100, 50)],              # out of store order, length 1, repeated
             [(store_n - 10, 10)], [(17, 1)],
             [(200, 100)], [(0, 250), (1000, 20)], [(3, 63), (900, 2), (50, 700)]]  # across 256-thread block boundaries
    for _ in range(4):
        k = int(rng.integers(1, 12))
        b = rng.integers(0, store_n, k)
        c = [int(rng.integers(0, min(store_n - x, 3000) + 1)) for x in b]
        cases.append(list(zip(b.tolist(), c)))
    for segs in cases:
        runs = np.concatenate([store[b:b + c] for b, c in segs]) if segs else store[:0]
        for layout in LAYOUTS:
            head = mc.host_vertices(runs, layout)
            for sel in (0, 1, 2):
                exp = np.concatenate([head, mc.host_vertices(_keep(live, sel), layout)])  # the runs FIRST, then the map part
                mc.same_vertices(ff.mesh_compose(sel, segs, layout), exp, layout, (segs, sel, layout))
            exp = np.concatenate([head, mc.host_vertices(_keep(live, 1), layout)])
            mc.same_vertices(_device_compose(ff, 1, segs, layout, len(exp)), exp, layout, ("device", segs, layout))
    # an invalid run: refused before any device work, the destination untouched
    dev = torch.full((64, 36), GUARD, dtype=torch.float32, device="cuda")
    for bad in ([(0, store_n + 1)], [(-1, 2)], [(store_n, 1)], [(3, -1)], [(0, 5), (store_n - 1, 2)]):
        with pytest.raises(api.DsmError) as e:
            ff.mesh_compose(1, bad, 0, dst_ptr=dev.data_ptr(), cap=64)
        assert e.value.code == api.DSM_E_INVALID
        assert (dev.cpu().numpy() == GUARD).all()
        with pytest.raises(api.DsmError) as e:
            ff.mesh_compose(1, bad, 1, cap=1 << 16)
        assert e.value.code == api.DSM_E_INVALID
    ff.close()


# ------------------------------------------------------------------ 3. capacity
def test_capacity(api):
    import torch
    rng = np.random.default_rng(3)
    ff = _engine(api)
    m = _records(rng, 9000, api)
    m["last_update"] = rng.integers(0, 4, len(m))
    ff.map_upload(m)
    ff.store_deactivate(2)
    store, _ = ff.store_download(0, ff.store_size())
    live = ff.map_download()
    lib = ff._lib
    for layout in LAYOUTS:
        words = mc.FLOATS[layout]
        for segs in ([], [(10, 700)], [(0, len(store))]):  # cap inside the map part, and (the last) inside the runs
            b = np.array([s[0] for s in segs] or [0], np.int32)
            c = np.array([s[1] for s in segs] or [0], np.int32)
            runs = np.concatenate([store[x:x + y] for x, y in segs]) if segs else store[:0]
            exp = np.concatenate([mc.host_vertices(runs, layout), mc.host_vertices(_keep(live, 1), layout)])
            need = len(exp)
            cap = need - 100 if len(runs) < len(store) else len(runs) - 100
            assert cap > 0
            n = C.c_int32(-1)
            host = np.full((cap + 64, words), GUARD, np.float32)
            rc = lib.dsm_mesh_compose(ff._h, 1, len(segs), b.ctypes.data, c.ctypes.data, layout, host.ctypes.data, 0, cap, C.byref(n))
            assert rc == api.DSM_E_CAPACITY and n.value == need
            assert (host[cap:] == GUARD).all()
            dev = torch.full((cap + 64, words), GUARD, dtype=torch.float32, device="cuda")
            n.value = -1
            rc = lib.dsm_mesh_compose(ff._h, 1, len(segs), b.ctypes.data, c.ctypes.data, layout, C.c_void_p(dev.data_ptr()), 1, cap, C.byref(n))
            assert rc == api.DSM_E_CAPACITY and n.value == need
            d = dev.cpu().numpy()
            assert (d[cap:] == GUARD).all()
            mc.same_vertices(d[:cap], exp[:cap], layout, ("prefix below cap", layout, segs))
            # exactly enough
            dev = torch.full((need + 1, words), GUARD, dtype=torch.float32, device="cuda")
            assert ff.mesh_compose(1, segs, layout, dst_ptr=dev.data_ptr(), cap=need) == need
            d = dev.cpu().numpy()
            mc.same_vertices(d[:need], exp, layout, ("exact", layout, segs))
            assert (d[need:] == GUARD).all()
            mc.same_vertices(ff.mesh_compose(1, segs, layout, cap=need), exp, layout, ("exact host", layout, segs))
    ff.close()


# ------------------------------------------------------------------ 4. indices
def test_indices(api):
    import torch
    ff = _engine(api)
    T = api.CLOUD_TILE
    for n in (0, 1, 65, T + 1):
        exp = mc.expect_faces(n)
        got = ff.mesh_indices(n)
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), exp), n
        for shift in (0, 1):  # 16-byte aligned (a thread per 16 bytes) and not (a thread per index)
            dev = torch.full((n * 12 + 8,), 0x7fffffff, dtype=torch.int32, device="cuda")
            ff.mesh_indices(n, dst_ptr=dev.data_ptr() + 4 * shift)
            d = dev.cpu().numpy()
            assert np.array_equal(d[shift:shift + n * 12].astype(np.int64).reshape(-1, 3), exp), (n, shift)
            assert (d[:shift] == 0x7fffffff).all() and (d[shift + n * 12:] == 0x7fffffff).all()
    with pytest.raises(api.DsmError) as e:
        ff.mesh_indices(715827883)
    assert e.value.code == api.DSM_E_INVALID
    ff.close()


# ------------------------------------------------------------------ 5. the node
def test_node_mesh(api, tmp_path):
    import torch
    import test_cpu
    from densesurfelmapping_amd import surfel_map, synth
    for case, gold in test_cpu._node_cases():
        cam, scene = node_state.camera_and_scene(case, synth)
        node = surfel_map.SurfelMap(cam, drift_free_poses=case["drift_free_poses"])
        for ev in synth.node_messages(cam, scene, case["frames"], **case["kw"]):
            node.feed(ev)
        before = node_state.digest(node_state.snapshot(node))
        assert before == gold["final_digest"]
        name = case["name"]
        # get_mesh(REF6), printed as the reference prints it, is the file save_mesh writes, which is the reference node's
        ref6 = node.get_mesh(api.MESH_VERTEX_REF6)
        n = len(ref6)
        assert n > 0
        ascii_path, printed_path = str(tmp_path / (name + ".ply")), str(tmp_path / (name + "_printed.ply"))
        node.save_mesh(ascii_path)
        mc.print_ref6(printed_path, ref6)
        # (NaN == NaN: iostreams print a NaN's sign bit, which the arithmetic does not define -- node_state.file_digest)
        canon = lambda path: open(path, "rb").read().replace(b"-nan", b"nan")
        assert canon(printed_path) == canon(ascii_path), name
        d = node_state.file_digest(ascii_path)
        assert d["sha256"] == gold["files"]["ply"]["sha256"] and d["bytes"] == gold["files"]["ply"]["bytes"], name
        # ... and the host corner function on the snapshot, in save_mesh's order
        snap = node_state.snapshot(node)
        s = np.concatenate([snap["attached"], snap["local"][snap["local"]["update_times"] >= 5]])
        mc.same_vertices(ref6, mc.host_vertices(s, mc.REF6), mc.REF6, (name, "ref6 vs host"))
        rgba = node.get_mesh(api.MESH_VERTEX_XYZ_RGBA8)
        mc.same_vertices(rgba, mc.host_vertices(s, mc.XYZ_RGBA8), mc.XYZ_RGBA8, (name, "rgba8 vs host"))
        # get_mesh_device == get_mesh
        for layout, host in ((api.MESH_VERTEX_REF6, ref6), (api.MESH_VERTEX_XYZ_RGBA8, rgba)):
            dev = torch.full((n + 4, mc.FLOATS[layout]), GUARD, dtype=torch.float32, device="cuda")
            assert node.get_mesh(layout, dst_ptr=dev.data_ptr(), cap=n + 4) == n
            dd = dev.cpu().numpy()
            mc.same_vertices(dd[:n], host, layout, (name, "device", layout))
            assert (dd[n:] == GUARD).all()
            with pytest.raises(api.DsmError) as e:
                node.get_mesh(layout, dst_ptr=dev.data_ptr(), cap=n - 1)
            assert e.value.code == api.DSM_E_CAPACITY
        # save_mesh_binary, parsed back: get_mesh's positions bit for bit, clamped colours, the reference's faces
        bin_path = str(tmp_path / (name + "_bin.ply"))
        node.save_mesh_binary(bin_path)
        pos, col, faces, head = mc.read_ply_binary(bin_path)
        assert head[1] == "format binary_little_endian 1.0"
        assert head[2:12] == open(ascii_path, "rb").read(600).decode("ascii", "replace").split("\n")[2:12]
        v6 = ref6.reshape(-1, 6)
        assert np.array_equal(pos.view(np.uint32), v6[:, :3].copy().view(np.uint32)), name
        assert np.array_equal(col, np.repeat(np.clip(v6[:, 3], 0, 255).astype(np.uint8)[:, None], 3, axis=1)), name
        assert np.array_equal(faces, mc.expect_faces(n)), name
        with pytest.raises(api.DsmError) as e:
            node.save_mesh_binary(str(tmp_path / "no_such_dir" / "m.ply"))
        assert e.value.code == api.DSM_E_INVALID
        # nothing changed
        assert node_state.digest(node_state.snapshot(node)) == before, name
        node.close()


def test_node_mesh_before_the_first_fuse(api, tmp_path):
    from densesurfelmapping_amd import surfel_map, synth
    node = surfel_map.SurfelMap(synth.NODE_CAM, drift_free_poses=3)
    with pytest.raises(api.DsmError) as e:
        node.get_mesh()
    assert e.value.code == api.DSM_E_STATE
    with pytest.raises(api.DsmError) as e:
        node.save_mesh_binary(str(tmp_path / "m.ply"))
    assert e.value.code == api.DSM_E_STATE
    node.close()


# ------------------------------------------------------------------ 6. one larger case
def test_large_map_order(api):
    """(1 << 20) + T + 5 records: more than 1024 tiles, so the scan takes a second trip round its loop; the order across
    workgroups.  151 MB of REF6 vertices: far below a 32-bit byte offset (the 64-bit offsets are checked by reading)."""
    rng = np.random.default_rng(11)
    n = (1 << 20) + api.CLOUD_TILE + 5
    ff = _engine(api, cap=n)
    m = _records(rng, n, api)
    ff.map_upload(m)
    mc.same_vertices(ff.mesh_compose(1, (), mc.REF6), mc.host_vertices(_keep(m, 1), mc.REF6), mc.REF6, "large ref6 mature")
    mc.same_vertices(ff.mesh_compose(2, (), mc.XYZ_RGBA8), mc.host_vertices(_keep(m, 2), mc.XYZ_RGBA8), mc.XYZ_RGBA8, "large rgba8 nonzero")
    ff.close()
