"""The voxel grid on the GPU (dsm_grid_compose, dsm_grid_inflate, dsm_surfel_map_grid*): index, occupied, inflated and cells
bit-identical, for host and device destinations, to the brute-force host checker of tests/grid_host.cpp, which evaluates the same
csrc/dsm_math.h functions as the kernels and which tests/test_cpu_grid.py pins to a float64 restatement of the definition."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_cases as gc
import mesh_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GUARD = 77  # bytes 0x4d: as a word 0x4d4d4d4d -- written nowhere by these cases (checked on the checker's outputs)
N_GUARD = 64
ALL = ("occupied", "inflated", "index", "cells")


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


def _engine(api, cap=1 << 15, flags=0):
    ff = api.FusionFunctions()
    ff.initialize(64, 32, 57.25, 55.5, 31.3, 15.7, 30.0, 0.3, surfel_capacity=cap, frame_slots=2, flags=flags)
    return ff


def _spec(api, s, inflate=None):
    """a grid_cases.Spec as the api's dsm_grid_spec"""
    return api.grid_spec(s.origin[:], s.voxel, gc.dims(s), s.inflate if inflate is None else inflate)


def _sizes(s, cells_cap):
    n_words, n_vox = gc.words(s) * s.ny * s.nz, s.nx * s.ny * s.nz
    return {"occupied": n_words, "inflated": n_words, "index": n_vox, "cells": cells_cap}


def _device_buffers(s, cells_cap, planes=ALL):
    """a torch byte buffer per plane with N_GUARD guard words behind it, all bytes GUARD"""
    import torch
    return {k: torch.full(((_sizes(s, cells_cap)[k] + N_GUARD) * 4,), GUARD, dtype=torch.uint8, device="cuda") for k in planes}


def _read_device(s, bufs, cells_cap, n_cells, what=""):
    out = {}
    shapes = {"occupied": (s.nz, s.ny, gc.words(s)), "inflated": (s.nz, s.ny, gc.words(s)), "index": (s.nz, s.ny, s.nx)}
    for k, t in bufs.items():
        a = t.cpu().numpy().view(np.int32 if k in ("index", "cells") else np.uint32)
        n = _sizes(s, cells_cap)[k]
        assert (a[n:].view(np.uint8) == GUARD).all(), (what, k, "guard words written")
        if k == "cells":
            written = min(n_cells, cells_cap)
            assert (a[written:n].view(np.uint8) == GUARD).all(), (what, "cells written past the count")
            out[k] = a[:written].copy()
        else:
            out[k] = a[:n].reshape(shapes[k]).copy()
    return out


def _grid_both(api, ff, select, segs, s, flags=0, what=""):
    """host destination and device destination (with guards): the same outputs; returns them"""
    sp = _spec(api, s)
    host = ff.grid(select, segs, sp, flags, planes=ALL)
    bufs = _device_buffers(s, host["n_cells"])
    n, nc = ff.grid(select, segs, sp, flags, dst_ptrs={k: t.data_ptr() for k, t in bufs.items()}, cells_cap=host["n_cells"])
    assert (n, nc) == (host["n_surfels"], host["n_cells"]), what
    gc.same_grids(_read_device(s, bufs, host["n_cells"], nc, what), host, (what, "device vs host destination"))
    # without the index plane the bits are splatted directly: the same bits
    gc.same_grids(ff.grid(select, segs, sp, flags, planes=("occupied", "inflated", "cells")), host, (what, "without index"))
    return host


def _check(api, ff, seq, select, segs, s, flags=0, what=""):
    got = _grid_both(api, ff, select, segs, s, flags, what)
    assert got["n_surfels"] == len(seq), (what, got["n_surfels"], len(seq))
    exp = gc.host_all(seq, s, flags, brute=True)
    gc.same_grids(got, exp, what)
    assert got["n_cells"] == len(exp["cells"])
    return got


# ------------------------------------------------------------------ 1. the crafted set
@pytest.mark.parametrize("grid", list(gc.ALL_GRIDS), ids=list(gc.ALL_GRIDS))
def test_crafted_set(api, grid):
    s = gc.with_inflate(gc.ALL_GRIDS[grid], 2)
    ff = _engine(api)
    m, names = gc.crafted_records(api.SURFEL_DTYPE, s)
    ff.map_upload(m)
    lo, hi, keep = gc.host_boxes(m, s)
    small, big = gc.tiers(lo, hi, keep)
    if grid in gc.MAIN_GRIDS:  # both tiers are populated
        assert small.sum() >= 10 and big.sum() >= 3, (small.sum(), big.sum())
        for name in ("through the whole grid", "inf size: the whole slab"):
            assert big[names.index(name)], name
    shown = {}
    for select in (1, 2):
        seq = gc.keep_select(m, select)
        for flags in (0, gc.CELLS_OF_INFLATED):
            got = _check(api, ff, seq, select, (), s, flags, what=("crafted", grid, select, flags))
        shown[select] = set(seq["update_times"][np.unique(got["index"][got["index"] >= 0])].tolist())
    if grid != "1x1x1":  # update_times 0 / 4 / 5 against select 1 and 2
        assert 5 in shown[1] and 4 not in shown[1] and 0 not in shown[1]
        assert 5 in shown[2] and 4 in shown[2] and 0 not in shown[2]
    ff.close()


# ------------------------------------------------------------------ 2. store runs, then the map part; 3. permutations
def test_store_runs_then_map(api):
    rng = np.random.default_rng(5)
    s = gc.with_inflate(gc.GRID_37, 3)
    ff = _engine(api)
    world = gc.grid_records(rng, 5000, api.SURFEL_DTYPE, s, spread=(-0.1, 1.1), sizes=(0.02, 0.3), scales=(1.0,))
    world["last_update"] = rng.integers(0, 9, len(world))
    ff.map_upload(world)
    for key in (3, 0, 7, 5):
        ff.store_deactivate(key)
    store_n = ff.store_size()
    store, _ = ff.store_download(0, store_n)
    live = ff.map_download()
    assert store_n > 1000 and len(live) > 1000
    cases = [[], [(0, store_n)], [(5, 0), (0, 0)],
             [(store_n - 1, 1), (0, 3), (100, 50), (7, 0), (100, 50)],        # out of store order, length 1, repeated, empty
             [(3, 63), (900, 2), (50, 700)], [(store_n - 300, 300), (0, 300)]]
    for segs in cases:
        runs = np.concatenate([store[b:b + c] for b, c in segs]) if segs else store[:0]
        for sel in ((0, 1, 2) if len(segs) in (0, 5) else (1,)):
            seq = np.concatenate([runs, gc.keep_select(live, sel)])  # the runs FIRST, then the map part
            got = _check(api, ff, seq, sel, segs, s, what=("runs", segs, sel))
            if sel == 0 and not segs:
                assert (got["index"] == -1).all() and not got["occupied"].any() and not got["inflated"].any() and got["n_cells"] == 0
                continue
            # the numbering is the mesh's and the renderer's: index i names hexagon i of mesh_compose's output
            ref6 = ff.mesh_compose(sel, segs, mc.REF6).reshape(-1, 6, 6)
            assert len(ref6) == len(seq)
            idx = np.unique(got["index"][got["index"] >= 0])
            assert len(idx) > 20
            centre = ref6[idx, :, :3].astype(np.float64).mean(1)
            pos = np.stack([seq["px"], seq["py"], seq["pz"]], 1).astype(np.float64)[idx]
            assert (np.linalg.norm(centre - pos, axis=1) <= 1e-3 * np.abs(seq["size"][idx].astype(np.float64)) + 1e-5).all(), (segs, sel)
    ff.close()


def test_permutation_gives_the_same_sets(api):
    rng = np.random.default_rng(12)
    s = gc.with_inflate(gc.GRID_70, 2)
    ff = _engine(api)
    m = np.concatenate([gc.grid_records(rng, 3000, api.SURFEL_DTYPE, s, ut=7), gc.crafted_records(api.SURFEL_DTYPE, s)[0]])
    ff.map_upload(m)
    first = _check(api, ff, gc.keep_select(m, 2), 2, (), s, what="as built")
    again = ff.grid(2, (), _spec(api, s), planes=ALL)
    for k in ALL:
        assert again[k].tobytes() == first[k].tobytes(), k  # the same compose twice: identical bytes
    p = m[rng.permutation(len(m))]
    ff.map_upload(p)
    second = _check(api, ff, gc.keep_select(p, 2), 2, (), s, what="permuted")
    for k in ("occupied", "inflated", "cells"):
        assert second[k].tobytes() == first[k].tobytes(), k
    assert not np.array_equal(second["index"], first["index"])
    ff.close()


# ------------------------------------------------------------------ 4. dsm_grid_inflate
def test_grid_inflate_device(api):
    import torch
    ff = _engine(api)
    rng = np.random.default_rng(3)
    for name, vox in gc.inflate_sets():
        nz, ny, nx = vox.shape
        bits = gc.pack(vox)
        dirty = bits.copy()
        dirty[..., -1] |= gc.pad_mask(nx) & rng.integers(0, 1 << 32, dirty[..., -1].shape, dtype=np.uint64).astype(np.uint32)
        src = torch.from_numpy(dirty.view(np.int32)).cuda()
        for r in (gc.INFLATE_RADII if not name.startswith("single") else (0, 1, 3, 16)):
            dst = torch.full(((bits.size + N_GUARD) * 4,), GUARD, dtype=torch.uint8, device="cuda")
            ff.grid_inflate((nx, ny, nz), r, src.data_ptr(), dst.data_ptr())
            a = dst.cpu().numpy().view(np.uint32)
            assert (a[bits.size:].view(np.uint8) == GUARD).all(), (name, r)
            assert np.array_equal(a[:bits.size].reshape(bits.shape), gc.host_inflate(bits, nx, r)), (name, r)  # (pad bits 0, dirty ones ignored)
        assert np.array_equal(src.cpu().numpy().view(np.uint32), dirty)
    # refusals: nothing written
    dst = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    src = torch.zeros(1024, dtype=torch.int32, device="cuda")
    for dims, r, a, b in (((8, 8, 8), 1, src.data_ptr(), src.data_ptr()), ((8, 8, 8), 17, src.data_ptr(), dst.data_ptr()), ((8, 8, 8), -1, src.data_ptr(), dst.data_ptr()),
                          ((0, 8, 8), 1, src.data_ptr(), dst.data_ptr()), ((8, 8, -1), 1, src.data_ptr(), dst.data_ptr()), ((8, 8, 8), 1, None, dst.data_ptr()),
                          ((8, 8, 8), 1, src.data_ptr(), None), ((1 << 14, 1 << 14, 2), 1, src.data_ptr(), dst.data_ptr()),
                          ((8, 8, 8), 1, src.data_ptr(), src.data_ptr() + 128), ((8, 8, 8), 1, src.data_ptr() + 252, src.data_ptr()),  # 256 bytes each: overlapping
                          ((8, 8, 8), 1, src.data_ptr(), dst.data_ptr() + 2)):                                                        # not 4-byte aligned
        with pytest.raises(api.DsmError) as e:
            ff.grid_inflate(dims, r, a, b)
        assert e.value.code == api.DSM_E_INVALID, (dims, r)
        assert (dst.cpu().numpy() == GUARD).all()
    ff.close()


# ------------------------------------------------------------------ 5. the cell list
def test_cell_list_and_capacity(api):
    import torch
    rng = np.random.default_rng(21)
    s = gc.with_inflate(gc.GRID_33, 1)
    ff = _engine(api)
    m = gc.grid_records(rng, 60, api.SURFEL_DTYPE, s, ut=7, spread=(0.0, 1.0), sizes=(0.01, 0.05))
    ff.map_upload(m)
    sp = _spec(api, s)
    for flags in (0, gc.CELLS_OF_INFLATED):
        exp = gc.host_all(m, s, flags)
        want = exp["cells"]
        assert 50 < len(want) < s.nx * s.ny * s.nz and (np.diff(want) > 0).all()
        got = ff.grid(2, (), sp, flags, planes=ALL)
        assert np.array_equal(got["cells"], want) and got["n_cells"] == len(want)
        src = gc.unpack(got["inflated" if flags else "occupied"], s.nx)
        assert np.array_equal(np.flatnonzero(src.ravel()), got["cells"])
        # the centres of the cells: the down-sampled cloud
        pts = api.grid_cell_centres(sp, got["cells"])
        z, y, x = np.unravel_index(got["cells"], src.shape)
        assert np.array_equal(pts, np.stack([gc.centres(s, 0)[x], gc.centres(s, 1)[y], gc.centres(s, 2)[z]], 1))
        for cap in (len(want), len(want) - 1, 0):
            # host destination
            cells = np.full(len(want) + N_GUARD, -7, np.int32)
            occ = np.zeros_like(exp["occupied"])
            st = api._GridPlanes(occ.ctypes.data, None, None, cells.ctypes.data, cap)
            n, nc = C.c_int32(-1), C.c_int32(-1)
            rc = ff._lib.dsm_grid_compose(ff._h, 2, 0, None, None, C.byref(sp), flags, C.byref(st), 0, C.byref(n), C.byref(nc))
            assert rc == (api.DSM_OK if cap == len(want) else api.DSM_E_CAPACITY), (flags, cap, rc)
            assert nc.value == len(want) and n.value == len(m)
            assert np.array_equal(cells[:cap], want[:cap]) and (cells[cap:] == -7).all()  # nothing past the cap
            assert np.array_equal(occ, exp["occupied"])                                    # the other planes are complete
            # device destination
            bufs = _device_buffers(s, cap, ("inflated", "cells"))
            st = api._GridPlanes(None, bufs["inflated"].data_ptr(), None, bufs["cells"].data_ptr(), cap)
            rc = ff._lib.dsm_grid_compose(ff._h, 2, 0, None, None, C.byref(sp), flags, C.byref(st), 1, C.byref(n), C.byref(nc))
            assert rc == (api.DSM_OK if cap == len(want) else api.DSM_E_CAPACITY) and nc.value == len(want)
            dev = _read_device(s, bufs, cap, nc.value, (flags, cap))
            assert np.array_equal(dev["cells"], want[:cap]) and np.array_equal(dev["inflated"], exp["inflated"])
        with pytest.raises(api.DsmError) as e:
            ff.grid(2, (), sp, flags, planes=("cells",), cells_cap=3)
        assert e.value.code == api.DSM_E_CAPACITY and e.value.n_cells == len(want)
    # cells alone, sized by the second call
    only = ff.grid(2, (), sp, planes=("cells",))
    assert set(only) == {"cells", "n_surfels", "n_cells"} and np.array_equal(only["cells"], gc.host_all(m, s)["cells"])
    ff.close()
    del torch


# ------------------------------------------------------------------ 6. past the launch caps; scratch regrowth
def test_small_tier_past_its_launch_cap(api):
    """300 000 tiny surfels into 16 x 16 x 16: more than the 16 384 workgroups x 16 surfels one trip of k_grid_splat covers, so its
    grid-stride loop wraps.  The surfels are laid along the grid in sequence order, a voxel holds the first that covers it: the
    surfels of the second trip are the only ones over the last eighth of the grid."""
    n = 300_000
    assert n > 16384 * 16 + 1024
    s = gc.with_inflate(gc.spec((-1.0, 2.0, 0.5), 0.125, (16, 16, 16)), 1)
    dtype = api.SURFEL_DTYPE
    rng = np.random.default_rng(33)
    a = np.zeros(n, dtype)
    cell = (np.arange(n, dtype=np.int64) * 4096) // n
    for k, (f, c) in enumerate((("px", cell % 16), ("py", cell // 16 % 16), ("pz", cell // 256))):
        a[f] = gc.centres(s, k)[c] + rng.uniform(-0.4, 0.4, n).astype(np.float32) * np.float32(s.voxel)
    nrm = rng.normal(size=(n, 3))
    a["nx"], a["ny"], a["nz"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).T
    a["size"] = rng.uniform(0.001, 0.02, n)
    a["update_times"] = 7
    lo, hi, keep = gc.host_boxes(a, s)
    small, big = gc.tiers(lo, hi, keep)
    assert small.sum() > 16384 * 16 + 1024 and not big.any()
    ff = _engine(api, cap=n + 1024)
    ff.map_upload(a)
    got = _check(api, ff, a, 2, (), s, what="300 000 tiny surfels")
    assert (got["index"] >= 0).mean() > 0.9 and (got["index"] > 16384 * 16).sum() >= 200
    ff.close()


def test_big_tier_run_loop_and_clear_past_their_caps(api):
    """2600 wide discs (more than the 2048 workgroups of k_grid_splat_big) behind 1 060 000 tiny surfels in one store run (more than
    the 4096 x 256 records one trip of k_grid_setup_run covers), in a 420 x 48 x 110 grid (2 217 600 voxels: more than the 8192 x 256
    elements one trip of k_grid_clear covers, and more than 8192 x 4 wave units of k_grid_bits).  Against the BOXED checker, which
    tests/test_cpu_grid.py shows equal to the brute-force one (that one would take minutes here), and which is compared with
    brute force on a sample of these very records."""
    dtype = api.SURFEL_DTYPE
    s = gc.with_inflate(gc.spec((-10.0, -2.0, 0.0), 0.25, (420, 48, 110)), 1)
    assert s.nx * s.ny * s.nz > 8192 * 256 + 65536
    n_tiny, n_big = 1_060_000, 2600
    assert n_tiny > 4096 * 256 + 1024 and n_big > 2048 + 256
    rng = np.random.default_rng(35)
    a = np.zeros(n_tiny + n_big, dtype)
    t = a[:n_tiny]  # tiny surfels in the slices z < 50, laid along the grid in sequence order
    cell = (np.arange(n_tiny, dtype=np.int64) * (420 * 48 * 50)) // n_tiny
    for k, (f, c) in enumerate((("px", cell % 420), ("py", cell // 420 % 48), ("pz", cell // (420 * 48)))):
        t[f] = gc.centres(s, k)[c] + rng.uniform(-0.4, 0.4, n_tiny).astype(np.float32) * np.float32(s.voxel)
    nrm = rng.normal(size=(n_tiny, 3))
    t["nx"], t["ny"], t["nz"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).T
    t["size"] = rng.uniform(0.001, 0.02, n_tiny)
    b = a[n_tiny:]  # discs of 9.5 voxels radius in the planes y = const, slices z >= 50: number j the only cover of the voxels at its right rim
    j = np.arange(n_big)
    b["px"] = s.origin[0] + (10.0 + (j // 48) * 7.3) * s.voxel
    b["py"] = gc.centres(s, 1)[j % 48]
    b["pz"] = s.origin[2] + 98.0 * s.voxel
    b["ny"] = 1.0
    b["size"] = 9.5 * s.voxel
    a["update_times"] = 7
    a["last_update"] = np.where(np.arange(len(a)) < n_tiny, 1, 0)
    lo, hi, keep = gc.host_boxes(a, s)
    small, big = gc.tiers(lo, hi, keep)
    assert small[:n_tiny].all() and big[n_tiny:].all()
    ff = _engine(api, cap=len(a) + 1024)
    ff.map_upload(a)
    begin, n = ff.store_deactivate(1)
    assert (begin, n) == (0, n_tiny) and ff.store_size() == n_tiny
    segs = [(0, n_tiny)]
    exp = gc.host_all(a, s, 0, brute=False)
    shown = np.unique(exp["index"][exp["index"] >= 0])
    assert (shown >= n_tiny).sum() == n_big and (shown[shown < n_tiny] > 4096 * 256).sum() > 1000  # every disc shows; so does the second trip of the run loop
    assert (exp["index"].ravel()[8192 * 256:] >= 0).sum() > 1000 and (exp["index"].ravel()[8192 * 256:] < 0).sum() > 1000
    # the box of THESE records loses nothing either: brute force on a sample of them (ten discs, 200 tiny surfels)
    sample = np.concatenate([a[:n_tiny][:: n_tiny // 200][:200], a[n_tiny:][:: n_big // 10][:10]])
    gc.same_grids(gc.host_grid(sample, s, brute=False), gc.host_grid(sample, s, brute=True), "boxed == brute on a sample")
    got = _grid_both(api, ff, 2, segs, s, what="past the caps")
    assert got["n_surfels"] == len(a)
    gc.same_grids(got, exp, "past the caps")
    ff.close()


def test_cell_list_past_its_launch_caps(api):
    """A 1 x 1500 x 1500 grid: one word per row, 2 250 000 words -- more than the 8192 workgroups x 256 words one trip of
    k_grid_cell_count / k_grid_cell_scatter covers, and 8790 tiles, more than the 1024 k_cloud_scan takes at a time.  A few surfels
    all over it, a disc through the whole grid among them; the cells of `occupied` and of `inflated`, against the brute-force checker."""
    dtype = api.SURFEL_DTYPE
    s = gc.with_inflate(gc.spec((0.25, -75.0, -75.0), 0.1, (1, 1500, 1500)), 2)
    trip = 8192 * 256
    assert gc.words(s) * s.ny * s.nz > trip + 65536 and (gc.words(s) * s.ny * s.nz + 255) // 256 > 8 * 1024
    rng = np.random.default_rng(61)
    a = gc.grid_records(rng, 60, dtype, s, ut=7, spread=(0.0, 1.0), sizes=(0.05, 3.0), scales=(1.0,))
    a["px"] = rng.uniform(0.2, 0.4, len(a))
    a["pz"][:20] = rng.uniform(65.0, 74.9, 20)          # a third of them in the slices of the second trip
    a[-1]["size"], a[-1]["nx"], a[-1]["ny"], a[-1]["nz"] = 500.0, 0.0, 0.6, 0.8  # through the whole grid
    ff = _engine(api)
    ff.map_upload(a)
    for flags in (0, gc.CELLS_OF_INFLATED):
        got = _check(api, ff, a, 2, (), s, flags, what=("cell list past the caps", flags))
        cells = got["cells"]
        assert (cells < trip).sum() > 1000 and (cells >= trip).sum() > 1000 and (np.diff(cells) > 0).all(), (len(cells), (cells >= trip).sum())
    ff.close()


def test_regrowth_on_one_handle(api):
    rng = np.random.default_rng(44)
    dtype = api.SURFEL_DTYPE
    ff = _engine(api)
    small_map = gc.grid_records(rng, 50, dtype, gc.GRID_32, ut=7)
    ff.map_upload(small_map)
    first = _check(api, ff, small_map, 2, (), gc.with_inflate(gc.GRID_32, 1), what="small")
    _check(api, ff, small_map, 2, (), gc.GRID_1, what="one voxel")
    larger = gc.grid_records(rng, 6000, dtype, gc.GRID_37)
    larger["last_update"] = np.arange(len(larger)) % 2
    ff.map_upload(larger)
    run = ff.store_deactivate(1)
    store, live = ff.store_download(0, ff.store_size())[0], ff.map_download()
    seq = np.concatenate([store[run[0]:run[0] + run[1]], gc.keep_select(live, 2)])
    got = _check(api, ff, seq, 2, [run], gc.with_inflate(gc.GRID_37, 5), gc.CELLS_OF_INFLATED, what="larger sequence and grid")
    assert (got["index"] >= run[1]).any() and ((got["index"] >= 0) & (got["index"] < run[1])).any()
    ff.map_upload(small_map)
    again = _check(api, ff, np.concatenate([store[run[0]:run[0] + run[1]], small_map]), 2, [run], gc.with_inflate(gc.GRID_32, 1), what="small again, with the run")
    only = _check(api, ff, small_map, 2, (), gc.with_inflate(gc.GRID_32, 1), what="small again")
    for k in ALL:
        assert only[k].tobytes() == first[k].tobytes(), k
    assert again["n_surfels"] == run[1] + len(small_map)
    ff.close()


# ------------------------------------------------------------------ 7. refusals
def test_invalid_arguments_touch_nothing(api):
    rng = np.random.default_rng(9)
    s = gc.with_inflate(gc.GRID_33, 2)
    ff = _engine(api)
    m = gc.grid_records(rng, 450, api.SURFEL_DTYPE, s, sizes=(0.01, 0.1))
    m["last_update"] = rng.integers(0, 3, len(m))
    ff.map_upload(m)
    ff.store_deactivate(1)
    store_n = ff.store_size()
    assert store_n > 100
    ff.frame_upload(0, rng.integers(0, 255, (32, 64)).astype(np.uint8), rng.uniform(0.5, 5.0, (32, 64)).astype(np.float32))
    before = (ff.store_download(0, store_n)[0].tobytes(), ff.map_download().tobytes(), ff.frame_planes(0)[0].tobytes(), ff.frame_planes(0)[1].tobytes())
    cap = 100
    bufs = _device_buffers(s, cap)
    ptrs = {k: t.data_ptr() for k, t in bufs.items()}
    host = {k: np.full(_sizes(s, cap)[k], 0x4d4d4d4d, np.uint32) for k in ALL}

    def spec_with(**kw):
        sp = _spec(api, s)
        for k, v in kw.items():
            if k.startswith("origin"):
                sp.origin[int(k[-1])] = v
            else:
                setattr(sp, k, v)
        return sp

    bad = [dict(segs=[(0, store_n + 1)]), dict(segs=[(-1, 2)]), dict(segs=[(store_n, 1)]), dict(segs=[(3, -1)]), dict(segs=[(0, 5), (store_n - 1, 2)]),
           dict(spec=spec_with(struct_size=32)), dict(spec=spec_with(struct_size=0)), dict(spec=spec_with(struct_size=40)),
           dict(spec=spec_with(origin0=float("nan"))), dict(spec=spec_with(origin1=float("inf"))), dict(spec=spec_with(origin2=float("-inf"))),
           dict(spec=spec_with(voxel=0.0)), dict(spec=spec_with(voxel=-0.1)), dict(spec=spec_with(voxel=float("nan"))), dict(spec=spec_with(voxel=float("inf"))),
           dict(spec=spec_with(nx=0)), dict(spec=spec_with(ny=0)), dict(spec=spec_with(nz=-3)),
           dict(spec=spec_with(nx=1 << 14, ny=1 << 14, nz=2)), dict(spec=spec_with(nx=(1 << 28) + 1, ny=1, nz=1)), dict(spec=spec_with(nx=1 << 30, ny=1 << 30, nz=1 << 30)),
           dict(spec=spec_with(inflate=-1)), dict(spec=spec_with(inflate=17)), dict(none=True), dict(alias=("occupied", "inflated")), dict(alias=("index", "cells")), dict(cells_cap=-1), dict(flags=2), dict(flags=0x80000001),
           dict(select=3)]
    for case in bad:
        kw = dict(select=1, segs=(), spec=_spec(api, s), flags=0, cells_cap=cap)
        none, alias = case.pop("none", False), case.pop("alias", None)
        kw.update(case)
        seg = np.asarray(kw["segs"], np.int32).reshape(-1, 2)
        b, c = (np.ascontiguousarray(seg[:, k]) if len(seg) else np.zeros(1, np.int32) for k in (0, 1))
        for dev in (1, 0):
            p = dict(ptrs if dev else {k: a.ctypes.data for k, a in host.items()})
            if alias:  # two planes the same memory
                p[alias[1]] = p[alias[0]]
            st = api._GridPlanes(*([None] * 4 if none else [p[k] for k in ALL]), kw["cells_cap"])
            n, nc = C.c_int32(-7), C.c_int32(-7)
            rc = ff._lib.dsm_grid_compose(ff._h, kw["select"], len(seg), b.ctypes.data, c.ctypes.data, C.byref(kw["spec"]), kw["flags"], C.byref(st), dev,
                                          C.byref(n), C.byref(nc))
            assert rc == api.DSM_E_INVALID, (case, dev, rc)
            assert (n.value, nc.value) == (-7, -7), case
        for k, t in bufs.items():
            assert (t.cpu().numpy() == GUARD).all(), (case, k)
        assert all((a == 0x4d4d4d4d).all() for a in host.values()), case
    # the Python wrapper raises the same
    with pytest.raises(api.DsmError) as e:
        ff.grid(1, (), spec_with(inflate=17))
    assert e.value.code == api.DSM_E_INVALID
    # ... the handle still composes, and nothing but scratch was written by any of it
    live = ff.map_download()
    store = ff.store_download(0, store_n)[0]
    _check(api, ff, np.concatenate([store[:50], gc.keep_select(live, 1)]), 1, [(0, 50)], s, what="after the refusals")
    assert (ff.store_download(0, store_n)[0].tobytes(), ff.map_download().tobytes(), ff.frame_planes(0)[0].tobytes(), ff.frame_planes(0)[1].tobytes()) == before
    ff.close()


def test_null_planes_and_guards(api):
    rng = np.random.default_rng(8)
    s = gc.with_inflate(gc.GRID_70, 1)
    ff = _engine(api)
    m = np.concatenate([gc.grid_records(rng, 150, api.SURFEL_DTYPE, s, sizes=(0.02, 0.3)), mc.random_records(rng, 300, api.SURFEL_DTYPE)])
    ff.map_upload(m)
    for flags in (0, gc.CELLS_OF_INFLATED):
        full = _check(api, ff, gc.keep_select(m, 2), 2, (), s, flags, what="all planes")
        assert 0.02 < (full["index"] >= 0).mean() < 0.98
        for planes in (("occupied",), ("inflated",), ("index",), ("cells",), ("occupied", "cells"), ("index", "inflated"), ("inflated", "cells")):
            host = ff.grid(2, (), _spec(api, s), flags, planes=planes)
            assert set(host) == set(planes) | {"n_surfels", "n_cells"}
            gc.same_grids(host, {k: full[k] for k in planes}, planes)
            assert host["n_cells"] == (full["n_cells"] if "cells" in planes else 0)
            # device: the planes asked for are written, the buffers of the others stay as they were
            bufs = _device_buffers(s, full["n_cells"])
            n, nc = ff.grid(2, (), _spec(api, s), flags, dst_ptrs={k: bufs[k].data_ptr() for k in planes}, cells_cap=full["n_cells"] if "cells" in planes else 0)
            got = _read_device(s, {k: bufs[k] for k in planes}, full["n_cells"], nc, planes)
            gc.same_grids(got, {k: full[k] for k in planes}, ("device", planes))
            for k in set(ALL) - set(planes):
                assert (bufs[k].cpu().numpy() == GUARD).all(), (planes, k)
    ff.close()


# ------------------------------------------------------------------ 8. the node
def _driftfree(links, root, rng_):
    """SurfelMap::get_driftfree_poses"""
    if root >= len(links):
        return []
    out, level = [root], [root]
    for _ in range(1, rng_):
        nxt = []
        for p in level:
            for q in links[p]:
                if q not in out:
                    nxt.append(q)
                    out.append(q)
        level = nxt
    return out


def test_node_grid(api, tmp_path):
    from densesurfelmapping_amd import msglog, surfel_map, synth
    import node_state
    case = node_state.SCENARIOS[0]  # one lap and a loop closure: warped and re-activated keyframes, deactivated a second time
    (cam, scene), dfp = node_state.camera_and_scene(case, synth), case["drift_free_poses"]
    events = list(synth.node_messages(cam, scene, case["frames"], **case["kw"]))
    log = str(tmp_path / "node.dsmlog")
    msglog.write_log(log, cam, dfp, iter(events))
    node = surfel_map.SurfelMap(cam, drift_free_poses=dfp)
    with pytest.raises(api.DsmError) as e:
        node.grid("all", centre=(0.0, 0.0, 0.0))
    assert e.value.code == api.DSM_E_STATE
    last = {}
    node.set_publish(("active",), lambda pub: last.update(pub))
    for ev in events:
        node.feed(ev)
    node.set_publish((), None)
    assert node.frames_fused > 40
    poses = [node.pose(i) for i in range(node.pose_count)]
    attached = [node.attached_surfels(i) for i in range(node.pose_count)]
    local = node.local_surfels()
    inactive = np.concatenate(attached)  # keyframe by keyframe in poses_database order: the mesh's order
    assert len(inactive) > 0 and (local["update_times"] >= 5).any()
    neighbor = [attached[p] for p in _driftfree([pp["links"] for pp in poses], last["relative_index"], 2 * dfp)
                if not poses[p]["is_local"] and poses[p]["n_attached"] > 0]
    seqs = {"active": local[local["update_times"] >= 5], "inactive": inactive,
            "all": np.concatenate([inactive, local[local["update_times"] >= 5]]),
            "neighbor": np.concatenate(neighbor + [local[local["update_times"] != 0]])}
    centre = node.last_pose()[:3, 3]
    voxel, dims = 1.0, (24, 8, 40)
    want_spec = api.grid_spec_around(centre, voxel, dims, 2)
    cells_seen = {}
    for kind, seq in seqs.items():
        got = node.grid(kind, voxel=voxel, dims=dims, inflate=2, planes=ALL)  # centre=None: the translation of the latest fuse's pose
        sp = got["spec"]
        assert list(sp.origin) == list(want_spec.origin) and (sp.nx, sp.ny, sp.nz, sp.inflate) == dims + (2,) and sp.voxel == want_spec.voxel
        # ... and a finer grid of the caller's own, round the middle of the surfels themselves
        pos = np.stack([seq["px"], seq["py"], seq["pz"]], 1)
        own = api.grid_spec_around(np.median(pos[np.isfinite(pos).all(1)], axis=0), 0.5, (24, 12, 24), 1)  # (freed slots of the map hold anything)
        for sp in (sp, own):
            got = node.grid(kind, spec=sp, planes=ALL)
            assert got["n_surfels"] == len(seq), kind
            exp = gc.host_all(seq, sp)
            gc.same_grids(got, exp, kind)
            assert got["n_cells"] == len(exp["cells"]), kind
            s = gc.as_spec(sp)
            bufs = _device_buffers(s, got["n_cells"])
            assert node.grid(kind, spec=sp, dst_ptrs={k: t.data_ptr() for k, t in bufs.items()}, cells_cap=got["n_cells"]) == (len(seq), got["n_cells"])
            gc.same_grids(_read_device(s, bufs, got["n_cells"], got["n_cells"], kind), got, (kind, "device"))
        cells_seen[kind] = got["n_cells"]
    print("node grids round the surfels' median: cells", cells_seen)
    assert all(v > 20 for v in cells_seen.values()), cells_seen
    # the grid is centred on the robot: the camera's voxel is the middle one
    mid = np.floor((centre - np.array(want_spec.origin[:])) / np.float32(voxel)).astype(int)
    assert all(abs(int(mid[a]) - dims[a] // 2) <= 1 for a in range(3)), (mid, dims)
    # a centre of the caller's own
    off = node.grid("all", voxel=voxel, dims=dims, centre=centre + np.float32(1.0), planes=("index",))
    assert list(off["spec"].origin) == list(api.grid_spec_around(centre + np.float32(1.0), voxel, dims).origin)
    gc.same_grids(off, gc.host_grid(seqs["all"], off["spec"]), "own centre")
    # "all" numbers its surfels as get_mesh does
    assert off["n_surfels"] == len(node.get_mesh())
    with pytest.raises(api.DsmError) as e:
        node.grid("raw")
    assert e.value.code == api.DSM_E_INVALID
    # too small a cell list: the count needed comes with the error
    full = node.grid("all", spec=want_spec, planes=("cells",))
    assert full["n_cells"] > 3
    with pytest.raises(api.DsmError) as e:
        node.grid("all", spec=want_spec, planes=("cells",), cells_cap=3)
    assert e.value.code == api.DSM_E_CAPACITY and e.value.n_cells == full["n_cells"]
    default = node.grid("all", voxel=voxel, dims=dims, inflate=1)
    node.close()
    # msglog --save-grid writes the same grid (a process of its own: that is what the command is)
    out = str(tmp_path / "grid.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "densesurfelmapping_amd.msglog", log, "--save-grid", out, "--grid-voxel", str(voxel), "--grid-dims"]
                       + [str(d) for d in dims] + ["--grid-inflate", "1"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["frames_fused"] > 40 and summary["grid_cells"] == default["n_cells"]
    saved = np.load(out)
    assert saved["origin"].tolist() == list(default["spec"].origin) and saved["dims"].tolist() == list(dims) and saved["voxel"] == np.float32(voxel)
    assert int(saved["inflate"]) == 1
    gc.same_grids({k: saved[k] for k in ("occupied", "inflated", "cells")}, default, "msglog --save-grid")
