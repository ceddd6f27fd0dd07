"""tests/maintenance_cases.py checked on the host: its float32 warp against the oracle's (oracle/dsm_oracle.c dsmo_warp), its
StoreModel against the oracle's extract and, operation by operation, against the stand-in engine of tests/node_hostemu.cpp;
the censuses that prove the crafted inputs hold what tests/test_gpu_maintenance.py is meant to meet; the validity of the
seeded schedules."""
import ctypes as C

import numpy as np
import pytest

import maintenance_cases as mc
from oracle import bindings as ob

NAN_CAP = 0.05


@pytest.fixture(scope="module")
def built(oracle_built):
    return oracle_built


def _crafted_maps():
    for n in mc.WARP_SIZES:
        yield "n%d" % n, mc.crafted_records(n, 11)[0]
    for name, off in mc.group_layouts().items():
        yield name, mc.layout_records(off, 23)[0]
    yield "big", mc.big_map()
    yield "schedule", mc.make_schedule(1)[0][1]
    for sizes, _, _ in mc.ERASE_CASES[:4]:
        yield "segments %s" % (sizes,), mc.segment_records(sizes, 5)


# ------------------------------------------------------------------ the warp
def test_numpy_warp_equals_the_oracle(built):
    fam = mc.family_matrices(5)
    for tag, s in _crafted_maps():
        for name, m in fam.items():
            want = ob.port_warp(s, m)
            assert mc.records_differ(mc.warp_np(s, m), want, True) == [], (tag, name)


def test_numpy_warp_equals_the_oracle_on_random_bits(built):
    rng = np.random.default_rng(1)
    s = mc.class_records(rng, "bits", 100000)
    s[::50] = mc.class_records(rng, "special_coords", 2000)
    for name in ("general", "rigid", "scale", "tiny_scale"):
        m = mc.matrix(name, rng)
        got, want = mc.warp_np(s, m), ob.port_warp(s, m)
        assert mc.records_differ(got, want, True) == [], name
        assert mc.nan_fraction([want]) <= NAN_CAP, name


def test_warp_census():
    fam = mc.family_matrices(5)
    assert set(fam) == set(mc.FAMILIES)
    classes, specials = set(), set()
    for n in mc.WARP_SIZES:
        s, cls = mc.crafted_records(n, 11)
        classes |= set(cls.tolist())
        if n >= 63:
            assert set(cls.tolist()) == set(range(len(mc.CLASSES))), n
        if n == 0:
            continue
        products, outs = [], []
        for m in fam.values():
            outs.append(mc.warp_np(s, m, products))
        # one case = one record set through every matrix family
        assert mc.nan_fraction(outs) <= NAN_CAP, (n, mc.nan_fraction(outs))
        if n >= 255:
            assert sum(int(mc.is_denormal(o[f]).sum()) for o in outs for f in mc.WARPED) >= 32, n
            assert sum(int(mc.is_denormal(p).sum()) for p in products) >= 32, n
        if n == 1000:
            sp = s[cls == mc.CLASSES.index("special_coords")]
            for f in mc.WARPED:
                specials |= set(sp[f].view(np.uint32).tolist())
            dm = s[cls == mc.CLASSES.index("deleted_match")]
            assert (dm["last_update"] == mc.KEY).all() and (dm["update_times"] == 0).any() and (dm["update_times"] < 0).any()
            assert set(mc.ODD_KEYS) <= set(s["last_update"].tolist()) and mc.ABSENT_KEY not in s["last_update"]
            pl = s[cls == mc.CLASSES.index("payload")]
            for f in ("size", "color", "weight"):
                assert np.isnan(pl[f]).any() and mc.is_denormal(pl[f]).any(), f
            for f in ("update_times", "last_update"):
                as_float = pl[f].view(np.float32)
                assert np.isnan(as_float).any() and mc.is_denormal(as_float).any(), f
            assert (pl["update_times"] > 0).all()
    assert classes == set(range(len(mc.CLASSES)))
    assert set(mc.SPECIALS.view(np.uint32).tolist()) <= specials
    # the matrix families are what their names say
    assert np.isnan(fam["nan"]).any() and np.isinf(fam["inf"]).any() and not fam["zero"].any()
    t = fam["denormal_t"][:3, 3]
    assert mc.is_denormal(t).sum() == 2 and np.signbit(t[1]) and t[1] == 0
    for name in ("scale", "shear", "general", "reflect"):
        r = fam[name][:3, :3].astype(np.float64)
        assert not np.allclose(r @ r.T, np.eye(3), atol=1e-3) or np.linalg.det(r) < 0, name


def test_group_census():
    layouts = mc.group_layouts()
    shapes = set()
    for name, off in layouts.items():
        assert off.dtype == np.int32 and off[0] == 0 and (np.diff(off) >= 0).all(), name
        shapes |= mc.layout_shapes(off)
        s, cls = mc.layout_records(off, 23)
        if len(s) >= 63:
            assert set(cls.tolist()) == set(range(len(mc.CLASSES))), name
        mats = mc.group_matrices(len(off) - 1, 3)
        assert mc.nan_fraction([mc.warp_groups_np(s, off, mats)]) <= NAN_CAP, name
        pats = mc.changed_patterns(off)
        assert pats["all"].all() and not pats["none"].any()
        if (np.diff(off) == 0).any():  # an empty group flagged changed between unchanged neighbours
            assert pats["only_empty"].any() and not pats["only_empty"][np.diff(off) > 0].any()
    assert shapes == set(mc.SHAPES), set(mc.SHAPES) - shapes
    assert len(layouts["thousands"]) - 1 == 3000 and mc.layout_shapes(layouts["single"]) == {"single"}
    d = np.diff(layouts["empty_edges"])
    assert any(d[g] == 0 and d[g - 1] > 0 and d[g + 1] > 0 for g in range(1, len(d) - 1))  # a lone empty group in the middle


def test_mark_pattern_census():
    s = mc.big_map()
    assert len(s) == mc.BIG_N > mc.MARK_CAP and (s["update_times"] > 0).all()
    run = np.flatnonzero(s["last_update"] == mc.RUN_KEY)
    assert run[0] < mc.MARK_CAP <= run[-1] and len(run) == run[-1] - run[0] + 1
    last = np.flatnonzero(s["last_update"] == mc.LAST_WORD_KEY)
    assert len(last) and last[0] // 64 == (mc.BIG_N - 1) // 64 and last[0] > mc.MARK_CAP
    assert not (s["last_update"] == mc.ABSENT_KEY).any()
    assert (mc.big_map_all(s)["last_update"] == mc.KEY).all() and mc.BIG_N > 2 * mc.EXTRACT_TRIP
    assert mc.BIG_N + 1000 > 2 * (1 << 18)  # with an earlier segment the store doubles twice in the all-marked call


def test_erase_census():
    shapes = set()
    for sizes, i, j in mc.ERASE_CASES:
        b, n = sum(sizes[:i]), sum(sizes[i:j])
        shapes |= mc.erase_shape(sum(sizes), b, n)
        s = mc.segment_records(sizes, 5)
        assert [int((s["last_update"] == g).sum()) for g in range(len(sizes))] == list(sizes)
    assert shapes == set(mc.ERASE_SHAPES), set(mc.ERASE_SHAPES) - shapes


# ------------------------------------------------------------------ the model
def test_model_extract_equals_the_oracle(built):
    for tag, s in _crafted_maps():
        for key in (mc.KEY, mc.ABSENT_KEY, 0) + mc.ODD_KEYS:
            model = mc.StoreModel(1 << 20)
            model.map_upload(s)
            out = model.map_extract(key)
            left, want = ob.port_extract_key(s, key)
            assert mc.records_differ(out, want, False) == [] and mc.records_differ(model.map, left, False) == [], (tag, key)
            if tag == "n1000" and key in (mc.KEY,) + mc.ODD_KEYS:
                assert len(out) > 0, key
            if key == mc.ABSENT_KEY:
                assert len(out) == 0


class StandIn:
    """the dsm_* entry points of tests/node_hostemu.cpp's CPU engine, called directly.  It has no dsm_map_extract and no
    dsm_map_append: those two go through the oracle's extract and an upload."""

    def __init__(self, path):
        from densesurfelmapping_amd import api
        self.lib = C.CDLL(path)
        cfg = api._Config()
        self.lib.dsm_config_init.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_float] * 6 + [C.c_int]
        assert self.lib.dsm_config_init(C.byref(cfg), 64, 32, 57.0, 57.0, 31.5, 15.5, 30.0, 0.3, 0) == 0
        self.h = C.c_void_p()
        assert self.lib.dsm_create(C.byref(cfg), C.byref(self.h)) == 0

    def close(self):
        self.lib.dsm_destroy(self.h)

    def map_upload(self, s):
        s = np.ascontiguousarray(s, mc.DT)
        assert self.lib.dsm_map_upload(self.h, s.ctypes.data_as(C.c_void_p), len(s)) == 0

    def map_download(self):
        n = C.c_int32(0)
        self.lib.dsm_map_size(self.h, C.byref(n))
        out = np.zeros(max(n.value, 1), mc.DT)
        assert self.lib.dsm_map_download(self.h, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)) == 0
        return out[:n.value]

    def map_warp(self, m):
        cm = np.ascontiguousarray(np.asarray(m, np.float32).T).ravel()
        assert self.lib.dsm_map_warp(self.h, cm.ctypes.data_as(C.c_void_p)) == 0

    def map_extract(self, key):
        left, out = ob.port_extract_key(self.map_download(), key)
        self.map_upload(left)
        return out

    def map_append(self, s):
        self.map_upload(np.concatenate([self.map_download(), np.asarray(s, mc.DT)]))

    def store_deactivate(self, key):
        b, n = C.c_int32(-1), C.c_int32(-1)
        assert self.lib.dsm_store_deactivate(self.h, key, C.byref(b), C.byref(n)) == 0
        return b.value, n.value

    def store_activate(self, b, n):
        assert self.lib.dsm_store_activate(self.h, b, n) == 0

    def store_erase(self, b, n):
        assert self.lib.dsm_store_erase(self.h, b, n) == 0

    def store_warp(self, off, mats, changed):
        off = np.ascontiguousarray(off, np.int32)
        cm = np.ascontiguousarray(np.asarray(mats, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1)
        ch = np.ascontiguousarray(changed, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert self.lib.dsm_store_warp(self.h, len(off) - 1, p(off), p(cm), p(ch)) == 0

    def store_size(self):
        n = C.c_int32(0)
        self.lib.dsm_store_size(self.h, C.byref(n))
        return n.value

    def store_download(self, b=0, n=None):
        n = self.store_size() - b if n is None else n
        s, c = np.zeros(max(n, 1), mc.DT), np.zeros((max(n, 1), 4), np.float32)
        assert self.lib.dsm_store_download(self.h, b, n, s.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)) == 0
        return s[:n], c[:n]


@pytest.mark.parametrize("seed", mc.SCHEDULE_SEEDS)
def test_schedule_model_equals_the_stand_in(node_hostemu_lib, seed):
    ops = mc.make_schedule(seed)
    count, shapes, final = mc.check_schedule(ops)
    assert len(ops) >= 60 and min(count.values()) >= 3, count
    assert mc.nan_fraction([final.map, final.store, final.cloud[:, :3]]) <= NAN_CAP
    assert 4500 <= len(ops[0][1]) <= 5500 and len(set(ops[0][1]["last_update"].tolist())) >= mc.SCHEDULE_KEYS
    # a warped segment's last point is stale in the cloud somewhere along the way, and the model says so at the end
    emu, model = StandIn(node_hostemu_lib), mc.StoreModel(mc.SCHEDULE_CAP)
    stale = 0
    for k, op in enumerate(ops):
        mc.same_result(op[0], mc.apply(emu, op), mc.apply(model, op))
        mc.same_state(emu, model, (seed, k, op[0]))
        if op[0] == "store_warp":
            stale += int((mc._bits(model.cloud[:, :3]) != mc._bits(mc.xyzi(model.store)[:, :3])).any(axis=1).sum())
    assert stale > 0
    emu.close()


def test_schedules_differ_and_cover_the_erase_shapes():
    shapes, orders = set(), set()
    for seed in mc.SCHEDULE_SEEDS:
        ops = mc.make_schedule(seed)
        shapes |= mc.check_schedule(ops)[1]
        orders.add(tuple(op[0] for op in ops))
    assert len(orders) == len(mc.SCHEDULE_SEEDS)
    assert {"tail_longer", "tail_shorter", "hole_at_0", "hole_at_end"} <= shapes, shapes


def test_check_schedule_refuses_invalid_orders():
    ops = mc.make_schedule(1)
    k = next(i for i, op in enumerate(ops) if op[0] == "store_erase" and op[2] > 1)
    bad = ops[:k] + [("store_erase", ops[k][1], ops[k][2] - 1)]
    with pytest.raises(AssertionError):
        mc.check_schedule(bad)
    k = next(i for i, op in enumerate(ops) if op[0] == "store_warp" and len(op[1]) > 1)
    off = ops[k][1].copy()
    off[-1] += 1
    with pytest.raises(AssertionError):
        mc.check_schedule(ops[:k] + [("store_warp", off, ops[k][2], ops[k][3])])
    with pytest.raises(AssertionError):
        mc.check_schedule(ops[:1] + [("map_append", np.zeros(mc.SCHEDULE_CAP, mc.DT))])


def test_comparison_helpers_excuse_nothing_but_a_warped_nan():
    rng = np.random.default_rng(0)
    a = mc.plain_records(rng, 8)
    b = a.copy()
    assert mc.records_differ(a, b, True) == []
    a["px"][0], b["px"][0] = np.array([0x7fc00000, 0xffc00001], np.uint32).view(np.float32)
    assert mc.records_differ(a, b, True) == [] and mc.records_differ(a, b, False) == [("px", 1, 0)]
    a["size"][3], b["size"][3] = np.array([0x7fc00000, 0x7fc00001], np.uint32).view(np.float32)
    assert mc.records_differ(a, b, True) == [("size", 1, 3)]
    b = a.copy()
    b["py"][2] = -b["py"][2]
    b["update_times"][5] += 1
    assert mc.records_differ(a, b, True) == [("py", 1, 2), ("update_times", 1, 5)]
    z = np.zeros(2, mc.DT)
    y = z.copy()
    y["nz"][1] = -0.0
    assert mc.records_differ(z, y, True) == [("nz", 1, 1)]
    c = mc.xyzi(a)
    d = c.copy()
    d[1, 3] = np.float32(np.nan)
    assert mc.cloud_differs(c, d, True) == [("i", 1, 1)] and mc.cloud_differs(c, c.copy(), False) == []


def test_frames_schedule_census(built):
    from densesurfelmapping_amd import synth
    cam = synth.TINY
    frames = list(synth.sequence(cam, synth.Scene(seed=31), mc.N_FRAMES))
    model = mc.StoreModel(1 << 16)
    stats = mc.frames_schedule(frames, ob.PortOracle(cam), model)
    print(stats)
    assert stats["refilled"] >= 1 and stats["shrunk"] >= 1 and stats["re_extracted"] > 0 and stats["stale"] == 2
    assert min(stats["segments"]) >= 64 and len(model.store) > 0
