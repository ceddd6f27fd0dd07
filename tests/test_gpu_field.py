"""The distance field on the GPU (dsm_grid_distance, dsm_field_compose, dsm_surfel_map_field*): dist2, nearest and distance
bit-identical, for host and device destinations, to the brute-force host checker of tests/field_host.cpp, which evaluates the
definition (csrc/dsm_math.h's field_key) directly and which tests/test_cpu_field.py pins to a numpy restatement."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import field_cases as fc
import grid_cases as gc

ROOT = fc.ROOT
pytestmark = pytest.mark.gpu

GUARD = 77  # bytes 0x4d: 0x4d4d as dist2 (19789 > 4096, not 65535), 0x4d4d4d4d as nearest (beyond any grid here) -- written nowhere by these cases
N_GUARD = 256  # guard bytes behind every plane
SUBSETS = [p for k in (1, 2) for p in itertools.combinations(fc.PLANES, k)]  # every proper subset of the planes but the empty one


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


def _buffers(n_vox, planes=fc.PLANES):
    """a torch byte buffer per plane with N_GUARD guard bytes behind it, all bytes GUARD"""
    import torch
    return {k: torch.full((n_vox * np.dtype(fc.TYPES[k]).itemsize + N_GUARD,), GUARD, dtype=torch.uint8, device="cuda") for k in planes}


def _read(bufs, shape, what=""):
    out = {}
    n_vox = int(np.prod(shape))
    for k, t in bufs.items():
        a = t.cpu().numpy()
        n = n_vox * np.dtype(fc.TYPES[k]).itemsize
        assert (a[n:] == GUARD).all(), (what, k, "guard bytes written")
        out[k] = a[:n].view(fc.TYPES[k]).reshape(shape).copy()
    return out


def _untouched(bufs, what=""):
    for k, t in bufs.items():
        assert (t.cpu().numpy() == GUARD).all(), (what, k, "written")


def _distance(ff, g, r, src, planes=fc.PLANES, what=""):
    """dsm_grid_distance on the device bit set `src` into guarded buffers: the planes asked for; the others stay untouched"""
    nx, ny, nz = g
    bufs = _buffers(nx * ny * nz)
    ff.grid_distance(g, r, fc.VOXEL, src.data_ptr(), {k: bufs[k].data_ptr() for k in planes})
    _untouched({k: bufs[k] for k in fc.PLANES if k not in planes}, what)
    return _read({k: bufs[k] for k in planes}, (nz, ny, nx), what)


def _upload(bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint32).view(np.int32)).cuda()


# ------------------------------------------------------------------ 1. a caller's bit set
@pytest.mark.parametrize("g", fc.GRIDS, ids=[fc.grid_id(g) for g in fc.GRIDS])
def test_callers_bit_set(api, g):
    ff = _engine(api)
    rng = np.random.default_rng(17)
    cases = [c for c in fc.case_list() if c[0] == g]
    assert {c[2] for c in cases} == set(fc.RADII) and len({c[1] for c in cases}) >= 15
    uploaded = {}
    for k, (_, name, r) in enumerate(cases):
        if name not in uploaded:
            bits = gc.pack(fc.sets(g)[name])
            dirty = fc.dirty_pads(bits, g[0], rng)
            assert g[0] % 32 == 0 or (dirty != bits).any()
            uploaded[name] = (_upload(bits), _upload(dirty), dirty)
        clean, dirty, dirty_host = uploaded[name]
        exp = fc.expected(g, name, r)
        fc.same_fields(_distance(ff, g, r, dirty, what=(g, name, r)), exp, (g, name, r, "garbage in the pad bits"))
        if g[0] % 32:
            fc.same_fields(_distance(ff, g, r, clean, what=(g, name, r)), exp, (g, name, r, "clean pad bits"))
        sub = SUBSETS[k % len(SUBSETS)]  # a NULL plane or two: the others are the same planes
        fc.same_fields(_distance(ff, g, r, dirty, sub, what=(g, name, r, sub)), {p: exp[p] for p in sub}, (g, name, r, sub))
    for name, (clean, dirty, dirty_host) in uploaded.items():  # the source is read only
        assert np.array_equal(dirty.cpu().numpy().view(np.uint32), dirty_host), name
    ff.close()


def test_every_subset_of_planes(api):
    g, name = (37, 21, 13), "random 0.05"
    ff = _engine(api)
    src = _upload(gc.pack(fc.sets(g)[name]))
    for r in (3, 64):
        exp = fc.expected(g, name, r)
        for sub in SUBSETS + [fc.PLANES]:
            fc.same_fields(_distance(ff, g, r, src, sub, what=(r, sub)), {p: exp[p] for p in sub}, (r, sub))
    # the voxel edge is read only for `distance`: without that plane anything goes
    nx, ny, nz = g
    bufs = _buffers(nx * ny * nz, ("dist2",))
    ff.grid_distance(g, 3, float("nan"), src.data_ptr(), {"dist2": bufs["dist2"].data_ptr()})
    fc.same_fields(_read(bufs, (nz, ny, nx)), {"dist2": fc.expected(g, name, 3)["dist2"]}, "NaN voxel, dist2 alone")
    # another edge: another table, the same dist2
    bufs = _buffers(nx * ny * nz)
    ff.grid_distance(g, 3, 0.1, src.data_ptr(), {k: t.data_ptr() for k, t in bufs.items()})
    got = _read(bufs, (nz, ny, nx))
    exp = fc.host_field(gc.pack(fc.sets(g)[name]), nx, 3, voxel=0.1)
    fc.same_fields(got, exp, "voxel 0.1")
    assert np.array_equal(got["distance"].view(np.uint32), api.field_distance_table(0.1, 3)[np.where(got["nearest"] >= 0, got["dist2"], 9)].view(np.uint32))
    ff.close()


# ------------------------------------------------------------------ 2. order independence
def test_twice_and_embedded(api):
    small, big, off, r = (37, 21, 13), (64, 64, 32), (10, 20, 9), 8
    assert all(r < off[a] and r < big[a] - (off[a] + small[a]) for a in range(3))  # R < the margin on every side
    ff = _engine(api)
    vox = fc.sets(small)["random 0.05"]
    src = _upload(gc.pack(vox))
    first, again = _distance(ff, small, r, src), _distance(ff, small, r, src)
    for k in fc.PLANES:
        assert first[k].tobytes() == again[k].tobytes(), k
    fc.same_fields(first, fc.host_field(gc.pack(vox), small[0], r), "37x21x13 at R 8")
    wide = np.zeros(big[::-1], bool)
    region = tuple(slice(off[a], off[a] + small[a]) for a in (2, 1, 0))
    wide[region] = vox
    got = _distance(ff, big, r, _upload(gc.pack(wide)))
    assert np.array_equal(got["dist2"][region], first["dist2"]) and np.array_equal(got["distance"][region].view(np.uint32), first["distance"].view(np.uint32))
    near = got["nearest"][region].astype(np.int64)
    have = near >= 0
    x, y, z = near % big[0] - off[0], near // big[0] % big[1] - off[1], near // (big[0] * big[1]) - off[2]
    assert np.array_equal(have, first["nearest"] >= 0) and np.array_equal(((z * small[1] + y) * small[0] + x)[have], first["nearest"][have])
    ff.close()


# ------------------------------------------------------------------ 3. a crafted map
def _map_with_store(api, ff, s, rng):
    m = np.concatenate([gc.crafted_records(api.SURFEL_DTYPE, s)[0], gc.grid_records(rng, 400, api.SURFEL_DTYPE, s, spread=(0.0, 1.0), sizes=(0.02, 0.3), scales=(1.0,))])
    m["last_update"] = np.arange(len(m)) % 3
    ff.map_upload(m)
    run = ff.store_deactivate(1)
    assert run[1] > 100
    return run, ff.store_download(0, ff.store_size())[0], ff.map_download()


def test_crafted_map(api):
    rng = np.random.default_rng(23)
    s = gc.GRID_37
    nx, ny, nz = gc.dims(s)
    ff = _engine(api)
    run, store, live = _map_with_store(api, ff, s, rng)
    before = (ff.store_download(0, ff.store_size())[0].tobytes(), ff.map_download().tobytes())
    for select, segs, r in ((1, (), 16), (2, (), 64), (2, [run], 16), (1, [(run[0] + 5, 40), (run[0], 3)], 3)):
        seq = np.concatenate([store[b:b + c] for b, c in segs] + [gc.keep_select(live, select)])
        occ = gc.host_grid(seq, s)["occupied"]
        assert 0.01 < gc.unpack(occ, nx).mean() < 0.9
        exp = fc.host_field(occ, nx, r, voxel=s.voxel)
        sp = api.grid_spec(s.origin[:], s.voxel, gc.dims(s), 0)
        host = ff.field(select, segs, sp, r)
        fc.same_fields(host, exp, (select, segs, r, "host destination"))
        bufs = _buffers(nx * ny * nz)
        n = ff.field(select, segs, sp, r, dst_ptrs={k: t.data_ptr() for k, t in bufs.items()})
        fc.same_fields(_read(bufs, (nz, ny, nx)), exp, (select, segs, r, "device destination"))
        bufs = _buffers(nx * ny * nz)
        assert ff.field(select, segs, sp, r, dst_ptrs={"nearest": bufs["nearest"].data_ptr()}) == n
        fc.same_fields(_read({"nearest": bufs["nearest"]}, (nz, ny, nx)), {"nearest": exp["nearest"]}, "nearest alone")
        _untouched({k: bufs[k] for k in ("dist2", "distance")})
        only = ff.field(select, segs, sp, r, planes=("distance",))
        assert set(only) == {"distance", "n_surfels"}
        fc.same_fields(only, {"distance": exp["distance"]}, "distance alone, host")
        # the same sequence and the same occupied set as dsm_grid_compose's; its inflation is the field's level set
        for radius in (1, 5, 16):
            if radius > r:
                continue
            grid = ff.grid(select, segs, api.grid_spec(s.origin[:], s.voxel, gc.dims(s), radius), planes=("occupied", "inflated"))
            assert grid["n_surfels"] == host["n_surfels"] == n == len(seq)
            assert np.array_equal(grid["occupied"], occ)
            assert np.array_equal(host["dist2"] <= radius * radius, gc.unpack(grid["inflated"], nx)), (select, segs, radius)
        have = host["nearest"] >= 0
        assert gc.unpack(occ, nx).ravel()[host["nearest"][have]].all() and (have == (host["dist2"] != fc.FAR)).all()
        # spec->inflate is validated and otherwise unused
        fc.same_fields(ff.field(select, segs, api.grid_spec(s.origin[:], s.voxel, gc.dims(s), 16), r), exp, "inflate 16 in the spec")
    assert (ff.store_download(0, ff.store_size())[0].tobytes(), ff.map_download().tobytes()) == before
    ff.close()


# ------------------------------------------------------------------ 4. refusals
def test_refusals_touch_nothing(api):
    import torch
    rng = np.random.default_rng(9)
    g = (33, 9, 5)
    nx, ny, nz = g
    n_vox, n_words = nx * ny * nz, 2 * ny * nz
    ff = _engine(api)
    s = gc.GRID_33
    run, store, live = _map_with_store(api, ff, s, rng)
    before = (ff.store_download(0, ff.store_size())[0].tobytes(), ff.map_download().tobytes())
    vox = rng.random((nz, ny, nx)) < 0.05
    src = torch.full((n_words * 4 + N_GUARD,), 0, dtype=torch.uint8, device="cuda")
    src[:n_words * 4] = torch.from_numpy(gc.pack(vox).view(np.uint8).ravel()).cuda()
    src_before = src.cpu().numpy().copy()
    bufs = _buffers(n_vox)
    p = {k: t.data_ptr() for k, t in bufs.items()}
    lib, h = ff._lib, ff._h

    def planes(**kw):
        q = dict(p, **kw)
        return api._FieldPlanes(q["dist2"], q["nearest"], q["distance"])

    ok = dict(dims=g, r=16, voxel=0.25, src=src.data_ptr(), planes=planes())
    bad = [dict(src=None), dict(planes=None), dict(dims=(0, 9, 5)), dict(dims=(33, -1, 5)), dict(dims=(33, 9, 0)),
           dict(dims=(1 << 13, 1 << 13, 2)), dict(dims=((1 << 26) + 1, 1, 1)), dict(dims=(1 << 30, 1 << 30, 1 << 30)),
           dict(r=0), dict(r=-1), dict(r=65), dict(r=1 << 20),
           dict(voxel=0.0), dict(voxel=-0.25), dict(voxel=float("nan")), dict(voxel=float("inf")),
           dict(planes=planes(dist2=None, nearest=None, distance=None)),
           dict(planes=planes(nearest=p["dist2"])), dict(planes=planes(distance=p["nearest"])), dict(planes=planes(distance=p["dist2"], nearest=None)),
           dict(planes=planes(dist2=src.data_ptr())), dict(planes=planes(nearest=src.data_ptr() + n_words * 4 - 4)),        # overlapping the source
           dict(planes=planes(distance=src.data_ptr() - n_vox * 4 + 4)), dict(src=p["nearest"] + 64),
           dict(src=src.data_ptr() + 2), dict(planes=planes(nearest=p["nearest"] + 2)), dict(planes=planes(distance=p["distance"] + 2)),
           dict(planes=planes(dist2=p["dist2"] + 1))]                                                                           # misaligned
    for case in bad:
        kw = dict(ok, **case)
        st = kw["planes"]
        rc = lib.dsm_grid_distance(h, *kw["dims"], kw["r"], kw["voxel"], kw["src"], None if st is None else C.byref(st))
        assert rc == api.DSM_E_INVALID, (case, rc)
        _untouched(bufs, case)
        assert np.array_equal(src.cpu().numpy(), src_before), case
    # dsm_field_compose: its own refusals, and the grid's
    sp_ok = lambda **kw: api.grid_spec(s.origin[:], s.voxel, gc.dims(s), 0)

    def spec_with(**kw):
        sp = sp_ok()
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp

    host = {k: np.full(n_vox, GUARD * 0x01010101, np.uint32).view(np.uint8)[:n_vox * np.dtype(fc.TYPES[k]).itemsize].copy() for k in fc.PLANES}
    okc = dict(select=1, segs=(), spec=sp_ok(), r=16, flags=0)
    badc = [dict(flags=1), dict(flags=2), dict(flags=0x80000000), dict(r=0), dict(r=65), dict(none=True), dict(alias=("dist2", "nearest")), dict(alias=("nearest", "distance")),
            dict(spec=spec_with(inflate=17)), dict(spec=spec_with(inflate=-1)), dict(spec=spec_with(struct_size=32)), dict(spec=spec_with(voxel=0.0)),
            dict(spec=spec_with(voxel=float("nan"))), dict(spec=spec_with(nx=0)), dict(spec=spec_with(nx=1 << 13, ny=1 << 13, nz=2)),
            dict(spec=None), dict(select=3), dict(segs=[(0, ff.store_size() + 1)]), dict(segs=[(-1, 2)])]
    for case in badc:
        kw = dict(okc)
        none, alias = case.pop("none", False), case.pop("alias", None)
        kw.update(case)
        seg = np.asarray(kw["segs"], np.int32).reshape(-1, 2)
        b, c = (np.ascontiguousarray(seg[:, k]) if len(seg) else np.zeros(1, np.int32) for k in (0, 1))
        for dev in (1, 0):
            q = dict(p if dev else {k: a.ctypes.data for k, a in host.items()})
            if alias:
                q[alias[1]] = q[alias[0]]
            st = api._FieldPlanes(*([None] * 3 if none else [q[k] for k in fc.PLANES]))
            n = C.c_int32(-7)
            rc = lib.dsm_field_compose(h, kw["select"], len(seg), b.ctypes.data, c.ctypes.data, None if kw["spec"] is None else C.byref(kw["spec"]), kw["r"],
                                       kw["flags"], C.byref(st), dev, C.byref(n))
            assert rc == api.DSM_E_INVALID and n.value == -7, (case, dev, rc)
        _untouched(bufs, case)
        assert all((a == GUARD).all() for a in host.values()), case
    for name, st in (("nearest", api._FieldPlanes(p["dist2"], p["nearest"] + 2, None)), ("dist2", api._FieldPlanes(p["dist2"] + 1, None, None))):  # misaligned device planes
        n = C.c_int32(-7)
        assert lib.dsm_field_compose(h, 1, 0, None, None, C.byref(sp_ok()), 16, 0, C.byref(st), 1, C.byref(n)) == api.DSM_E_INVALID, name
        _untouched(bufs, name)
    with pytest.raises(api.DsmError) as e:  # the Python wrappers raise the same
        ff.field(1, (), sp_ok(), 65)
    assert e.value.code == api.DSM_E_INVALID
    with pytest.raises(api.DsmError) as e:
        ff.grid_distance(g, 16, 0.25, src.data_ptr(), {})
    assert e.value.code == api.DSM_E_INVALID
    # dsm_grid_compose still refuses what it refused
    with pytest.raises(api.DsmError) as e:
        ff.grid(1, (), spec_with(inflate=17))
    assert e.value.code == api.DSM_E_INVALID
    # ... and the handle still works: both entry points, nothing but scratch written by any of it
    got = _distance(ff, g, 16, src[:n_words * 4].view(torch.int32))
    fc.same_fields(got, fc.host_field(gc.pack(vox), nx, 16), "after the refusals")
    seq = np.concatenate([store[run[0]:run[0] + 50], gc.keep_select(live, 1)])
    fc.same_fields(ff.field(1, [(run[0], 50)], sp_ok(), 16), fc.host_field(gc.host_grid(seq, s)["occupied"], nx, 16, voxel=s.voxel), "compose after the refusals")
    assert (ff.store_download(0, ff.store_size())[0].tobytes(), ff.map_download().tobytes()) == before
    ff.close()


# ------------------------------------------------------------------ 5. scratch regrowth
def test_regrowth_on_one_handle(api):
    rng = np.random.default_rng(44)
    ff = _engine(api)
    small, large = (2, 3, 4), (64, 64, 8)
    first = _distance(ff, small, 3, _upload(gc.pack(fc.sets(small)["random 0.5"])))
    fc.same_fields(first, fc.expected(small, "random 0.5", 3), "small")
    fc.same_fields(_distance(ff, large, 16, _upload(gc.pack(fc.sets(large)["random 0.05"]))), fc.host_field(gc.pack(fc.sets(large)["random 0.05"]), 64, 16), "largest")
    again = _distance(ff, small, 3, _upload(gc.pack(fc.sets(small)["random 0.5"])))
    for k in fc.PLANES:
        assert again[k].tobytes() == first[k].tobytes(), k
    # the composed form grows the same scratch: a small grid, a larger one, the small one again
    m = gc.grid_records(rng, 300, api.SURFEL_DTYPE, gc.GRID_37, ut=7, spread=(0.0, 1.0), sizes=(0.02, 0.3))
    ff.map_upload(m)
    for s, r in ((gc.GRID_32, 3), (gc.GRID_37, 64), (gc.GRID_1, 1), (gc.GRID_32, 3)):
        exp = fc.host_field(gc.host_grid(m, s)["occupied"], s.nx, r, voxel=s.voxel)
        fc.same_fields(ff.field(2, (), api.grid_spec(s.origin[:], s.voxel, gc.dims(s), 0), r), exp, (gc.dims(s), r))
    ff.close()


# ------------------------------------------------------------------ 6. the node and msglog
def test_node_field(api, tmp_path):
    from densesurfelmapping_amd import msglog, surfel_map, synth
    import node_state
    case = node_state.SCENARIOS[0]  # one lap and a loop closure, as tests/test_gpu_grid.py's node test
    (cam, scene), dfp = node_state.camera_and_scene(case, synth), case["drift_free_poses"]
    events = list(synth.node_messages(cam, scene, case["frames"], **case["kw"]))
    log = str(tmp_path / "node.dsmlog")
    msglog.write_log(log, cam, dfp, iter(events))
    node = surfel_map.SurfelMap(cam, drift_free_poses=dfp)
    with pytest.raises(api.DsmError) as e:
        node.field("all", centre=(0.0, 0.0, 0.0))
    assert e.value.code == api.DSM_E_STATE
    for ev in events:
        node.feed(ev)
    assert node.frames_fused > 40
    voxel, dims, r = 1.0, (24, 8, 40), 5
    reached = {}
    for kind in ("all", "active", "inactive", "neighbor"):
        grid = node.grid(kind, voxel=voxel, dims=dims, planes=("occupied",))
        got = node.field(kind, voxel=voxel, dims=dims, max_dist=r)  # centre=None: the translation of the latest fuse's pose
        sp = got["spec"]
        assert list(sp.origin) == list(grid["spec"].origin) and (sp.nx, sp.ny, sp.nz) == dims and got["n_surfels"] == grid["n_surfels"]
        exp = fc.host_field(grid["occupied"], dims[0], r, voxel=voxel)
        fc.same_fields(got, exp, kind)
        bufs = _buffers(dims[0] * dims[1] * dims[2])
        assert node.field(kind, spec=sp, max_dist=r, dst_ptrs={k: t.data_ptr() for k, t in bufs.items()}) == got["n_surfels"]
        fc.same_fields(_read(bufs, dims[::-1], kind), exp, (kind, "device"))
        reached[kind] = int((got["nearest"] >= 0).sum())
    print("node fields: voxels with an occupied voxel within", r, reached)
    assert all(v > 20 for v in reached.values()), reached
    with pytest.raises(api.DsmError) as e:
        node.field("raw")
    assert e.value.code == api.DSM_E_INVALID
    default = node.field("all", voxel=voxel, dims=dims, max_dist=7)
    node.close()
    # msglog --save-field writes the same planes (a process of its own: that is what the command is)
    out = str(tmp_path / "field.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "densesurfelmapping_amd.msglog", log, "--save-field", out, "--grid-voxel", str(voxel), "--grid-dims"]
                         + [str(d) for d in dims] + ["--field-max-dist", "7"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    assert summary["frames_fused"] > 40 and summary["field_near"] == int((default["dist2"] != fc.FAR).sum())
    saved = np.load(out)
    assert saved["origin"].tolist() == list(default["spec"].origin) and saved["dims"].tolist() == list(dims) and saved["voxel"] == np.float32(voxel)
    assert int(saved["max_dist"]) == 7 and set(saved.files) == {"origin", "voxel", "dims", "max_dist", "dist2", "nearest", "distance"}
    fc.same_fields({k: saved[k] for k in fc.PLANES}, default, "msglog --save-field")
