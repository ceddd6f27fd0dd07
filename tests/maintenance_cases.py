"""Inputs and the reference for the map maintenance that runs between frames: the loop-closure warp in its three forms
(dsm_map_warp, dsm_warp_grouped_device, dsm_store_warp) and the active-set moves (dsm_map_extract / _append,
dsm_store_deactivate / _activate / _erase / _download).

Built from numpy alone, never from the product (no GPU, no torch):

  * warp_np: surfel_map.cpp:681-789 restated in float32, one rounded numpy operation per operation of the reference's
    products -- o_i = ((m_i0 p0 + m_i1 p1) + m_i2 p2) + m_i3 1.0f, w_i = (m_i0 v0 + m_i1 v1) + m_i2 v2;
  * StoreModel: the map, the inactive store and its XYZI cloud as numpy arrays, with the rules of surfel_map.cpp:1456-1595
    (a removed surfel's slot stays in the map, deleted, until the next fuse compacts it) and of surfel_map.cpp:742 (the
    last point of a warped patch keeps its stale position in the cloud);
  * records the fuse never produces, matrices that are not rigid, group layouts at every offset of a wave trip, mark
    patterns, erase shapes, seeded schedules over the nine operations;
  * a census of every crafted input, computed from the reference alone (tests/test_cpu_maintenance.py asserts it).
"""
import numpy as np

from oracle import bindings as ob

F32 = np.float32
DT = ob.SURFEL_DTYPE
WARPED = ("px", "py", "pz", "nx", "ny", "nz")
UNTOUCHED = ("size", "color", "weight", "update_times", "last_update")
INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)
FLT_MIN = float(np.finfo(F32).tiny)  # the smallest normal

KEY = 7               # the key the crafted maps are extracted by
ODD_KEYS = (-1, INT_MIN, INT_MAX)
ABSENT_KEY = 12345


class CapacityError(Exception):
    """what the device reports as DSM_E_CAPACITY"""


# ---------------------------------------------------------------------------------------------------------------------
# the warp

def warp_np(s, m, products=None):
    """surfel_map.cpp:761-783 (and 711-732) on a copy of `s`; m: 4x4 row-major.  products: a list that receives every
    intermediate float32 array (the census counts the denormal ones)."""
    m = np.asarray(m, F32).reshape(4, 4)
    out = s.copy()
    p = [s["px"], s["py"], s["pz"]]
    v = [s["nx"], s["ny"], s["nz"]]
    one = F32(1.0)
    with np.errstate(all="ignore"):
        for i in range(3):
            a, b, c, d = m[i, 0] * p[0], m[i, 1] * p[1], m[i, 2] * p[2], m[i, 3] * one
            ab = a + b
            abc = ab + c
            out[WARPED[i]] = abc + d
            e, f, g = m[i, 0] * v[0], m[i, 1] * v[1], m[i, 2] * v[2]
            ef = e + f
            out[WARPED[3 + i]] = ef + g
            if products is not None:
                products += [a, b, c, ab, abc, e, f, g, ef]
    for x in (out[f] for f in WARPED):
        assert x.dtype == F32
    return out


def xyzi(s):
    """the cloud point of a record (surfel_map.cpp:1485-1490, 734-739)"""
    return np.stack([s["px"], s["py"], s["pz"], s["color"]], axis=1).astype(F32) if len(s) else np.zeros((0, 4), F32)


def is_denormal(x):
    a = np.abs(np.asarray(x, F32))
    return (a > 0) & (a < F32(FLT_MIN))


# ---------------------------------------------------------------------------------------------------------------------
# the model

class StoreModel:
    """The map, the store and the store's cloud.  `*_t` marks values that went through warp arithmetic since they were
    uploaded: only there may a NaN's sign and payload differ between two correct implementations."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.map, self.map_t = np.zeros(0, DT), np.zeros(0, bool)
        self.store, self.store_t = np.zeros(0, DT), np.zeros(0, bool)
        self.cloud, self.cloud_t = np.zeros((0, 4), F32), np.zeros(0, bool)

    def map_upload(self, s):
        self.map, self.map_t = np.array(s, DT), np.zeros(len(s), bool)

    def map_set(self, s):
        """the map after a fuse (the reference's own result): every value may have gone through arithmetic"""
        self.map, self.map_t = np.array(s, DT), np.ones(len(s), bool)

    def map_warp(self, m):
        self.map = warp_np(self.map, m)
        self.map_t[:] = True

    def map_extract(self, key, with_marks=False):
        hit = (self.map["update_times"] > 0) & (self.map["last_update"] == key)
        out, out_t = self.map[hit].copy(), self.map_t[hit].copy()
        self.map["update_times"][hit] = 0  # the slot stays until the next fuse
        return (out, out_t) if with_marks else out

    def map_append(self, s, marks=None):
        if len(self.map) + len(s) > self.capacity:
            raise CapacityError
        self.map = np.concatenate([self.map, np.asarray(s, DT)])
        self.map_t = np.concatenate([self.map_t, np.zeros(len(s), bool) if marks is None else marks])

    def store_deactivate(self, key):
        out, out_t = self.map_extract(key, with_marks=True)
        begin = len(self.store)
        self.store, self.store_t = np.concatenate([self.store, out]), np.concatenate([self.store_t, out_t])
        self.cloud, self.cloud_t = np.concatenate([self.cloud, xyzi(out)]), np.concatenate([self.cloud_t, out_t])
        return begin, len(out)

    def store_activate(self, begin, n):
        assert 0 <= begin and 0 <= n and begin + n <= len(self.store)
        self.map_append(self.store[begin:begin + n], self.store_t[begin:begin + n])

    def store_erase(self, begin, n):
        assert 0 <= begin and 0 <= n and begin + n <= len(self.store)
        keep = np.ones(len(self.store), bool)
        keep[begin:begin + n] = False
        self.store, self.store_t = self.store[keep], self.store_t[keep]
        self.cloud, self.cloud_t = self.cloud[keep], self.cloud_t[keep]

    def store_warp(self, offsets, mats, changed):
        assert offsets[0] == 0 and offsets[-1] == len(self.store) or len(offsets) == 1
        for g in range(len(offsets) - 1):
            b, e = int(offsets[g]), int(offsets[g + 1])
            if not changed[g] or e == b:
                continue
            self.store[b:e] = warp_np(self.store[b:e], mats[g])
            self.store_t[b:e] = True
            self.cloud[b:e - 1] = xyzi(self.store[b:e - 1])  # [&front, &back): the last point keeps its position
            self.cloud_t[b:e - 1] = True

    def store_download(self, begin, n):
        return self.store[begin:begin + n].copy(), self.cloud[begin:begin + n].copy()


def warp_groups_np(s, offsets, mats):
    """dsm_warp_grouped_device: every group by its matrix"""
    out = s.copy()
    for g in range(len(offsets) - 1):
        b, e = int(offsets[g]), int(offsets[g + 1])
        if e > b:
            out[b:e] = warp_np(s[b:e], mats[g])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# comparison

def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def records_differ(got, want, touched):
    """[(field, count, first index)] of the records that differ.  Warped fields of touched records: bit-equal or both NaN
    (conftest.fields_equal's rule); everything else -- the five fields a warp moves untouched, and all eleven of an untouched
    record -- by its raw bytes."""
    assert got.dtype == DT and want.dtype == DT
    if len(got) != len(want):
        return [("len", len(got), len(want))]
    touched = np.broadcast_to(np.asarray(touched, bool), (len(want),))
    bad = []
    for f in DT.names:
        g, w = _bits(got[f]), _bits(want[f])
        same = g == w
        if f in WARPED:
            same |= touched & np.isnan(got[f]) & np.isnan(want[f])
        if not same.all():
            bad.append((f, int((~same).sum()), int(np.flatnonzero(~same)[0])))
    return bad


def cloud_differs(got, want, touched):
    if got.shape != want.shape:
        return [("shape", got.shape, want.shape)]
    touched = np.broadcast_to(np.asarray(touched, bool), (len(want),))
    bad = []
    for k in range(4):
        same = _bits(got[:, k]) == _bits(want[:, k])
        if k < 3:
            same |= touched & np.isnan(got[:, k]) & np.isnan(want[:, k])
        if not same.all():
            bad.append(("xyzi"[k], int((~same).sum()), int(np.flatnonzero(~same)[0])))
    return bad


def same_result(name, got, want, touched=True):
    """what an operation hands back"""
    if name == "map_extract":
        assert records_differ(np.asarray(got, DT), want, touched) == [], name
    elif name == "store_deactivate":
        assert tuple(got) == tuple(want), (name, got, want)
    elif name == "store_download":
        assert records_differ(np.asarray(got[0], DT), want[0], touched) == [] and cloud_differs(got[1], want[1], touched) == [], name


def same_state(engine, model, tag):
    assert records_differ(np.asarray(engine.map_download(), DT), model.map, model.map_t) == [], tag
    s, c = engine.store_download()
    assert engine.store_size() == len(model.store), tag
    assert records_differ(np.asarray(s, DT), model.store, model.store_t) == [], tag
    assert cloud_differs(c, model.cloud, model.cloud_t) == [], tag


def nan_fraction(arrays):
    """share of NaN among the float values of the reference results in `arrays` (record arrays: the six warped fields)"""
    n = bad = 0
    for a in arrays:
        if a.dtype == DT:
            for f in WARPED:
                n += a[f].size
                bad += int(np.isnan(a[f]).sum())
        else:
            n += a.size
            bad += int(np.isnan(a).sum())
    return bad / max(n, 1)


# ---------------------------------------------------------------------------------------------------------------------
# records

CLASSES = ("plain", "bits", "deleted_match", "key_odd", "special_coords", "payload", "tiny")
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80012345, 0x007fffff, 0x7f7fffff, 0xff7fffff, 0x7f800000,
                     0xff800000, 0x7fc00000], np.uint32).view(F32)  # +-0, denormals, +-FLT_MAX, +-inf, NaN
# NaN payloads (quiet and signalling, either sign) and denormal bits for the float fields a warp does not touch
PAYLOAD_F = np.array([0x7fc12345, 0xffc00001, 0x7fa00000, 0xff800001, 0x00000001, 0x807fffff], np.uint32).view(F32)
# ints whose bits read as signalling NaNs or denormals
PAYLOAD_UT = np.array([0x7fa00000, 0x7f800001, 0x00000123, 0x007fffff], np.uint32).view(np.int32)  # (all positive: live)
PAYLOAD_LU = np.array([0x7fa00000, 0xffa00000, 0x00000123, 0x807fffff], np.uint32).view(np.int32)


def plain_records(rng, n, keys=(0, 1, 2, 3, KEY)):
    s = np.zeros(n, DT)
    for f in ("px", "py", "pz"):
        s[f] = rng.uniform(-5, 5, n)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True) + 1e-30
    s["nx"], s["ny"], s["nz"] = nrm.T.astype(F32)
    s["size"] = rng.uniform(0.01, 0.3, n)
    s["color"] = rng.integers(0, 256, n)
    s["weight"] = rng.uniform(0.1, 1.0, n)
    s["update_times"] = rng.integers(1, 30, n)
    s["last_update"] = rng.choice(np.asarray(keys, np.int32), n) if n else 0
    return s


def class_records(rng, name, n, key=KEY):
    s = plain_records(rng, n)
    if name == "bits":  # arbitrary bit patterns in all eleven words
        s = rng.integers(0, 1 << 32, (n, 11), dtype=np.uint64).astype(np.uint32).view(DT).reshape(n)
    elif name == "deleted_match":  # a deleted slot that still carries the key
        s["update_times"] = rng.choice(np.array([0, 0, -1, INT_MIN], np.int32), n)
        s["last_update"] = key
    elif name == "key_odd":
        s["last_update"] = rng.choice(np.array(ODD_KEYS, np.int32), n)
    elif name == "special_coords":
        for f in WARPED:
            pick = rng.random(n) < 0.3
            w = np.array([3, 3, 3, 3, 3, 3, 3, 2, 2, 1], float)
            s[f][pick] = rng.choice(SPECIALS, int(pick.sum()), p=w / w.sum())
    elif name == "payload":
        for f in ("size", "color", "weight"):
            s[f] = rng.choice(PAYLOAD_F, n)
        s["update_times"] = rng.choice(PAYLOAD_UT, n)
        s["last_update"] = rng.choice(np.concatenate([PAYLOAD_LU, np.array([key], np.int32)]), n)
    elif name == "tiny":  # products and sums below the smallest normal
        for f in WARPED:
            s[f] = (rng.uniform(0.05, 4.0, n) * rng.choice([-1.0, 1.0], n) * FLT_MIN).astype(F32)
        s["last_update"] = key
    else:
        assert name == "plain"
    return s


def crafted_records(n, seed, key=KEY):
    """(records, class index per record): the classes interleaved at random, each n // 7 or one more times"""
    rng = np.random.default_rng([seed, n])
    cls = rng.permutation((np.arange(n) + seed) % len(CLASSES))
    s = np.zeros(n, DT)
    for c, name in enumerate(CLASSES):
        idx = np.flatnonzero(cls == c)
        s[idx] = class_records(rng, name, len(idx), key)
    return s, cls


WARP_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


# ---------------------------------------------------------------------------------------------------------------------
# matrices

def rigid(rng, scale=0.4):
    a = rng.normal(size=3) * scale
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    m[:3, 3] = rng.normal(size=3) * 0.3
    return m.astype(F32)


FAMILIES = ("identity", "rigid", "scale", "shear", "zero", "nan", "inf", "denormal_t", "general", "huge", "reflect", "tiny_scale")
FINITE_FAMILIES = ("rigid", "scale", "shear", "denormal_t", "general", "reflect")  # (every one moves every point)


def matrix(name, rng):
    m = rigid(rng)
    if name == "identity":
        m = np.eye(4, dtype=F32)
    elif name == "scale":
        m[:3, :3] = (m[:3, :3] * np.array([2.5, 0.5, -3.0], F32)[None, :]).astype(F32)
    elif name == "shear":
        m[:3, :3] = np.array([[1, 0.75, -0.3], [0, 1, 1.5], [0, 0, 1]], F32)
    elif name == "zero":
        m = np.zeros((4, 4), F32)
    elif name == "nan":
        m[2, 0] = np.nan
    elif name == "inf":
        m[1, 1], m[0, 3] = np.inf, -np.inf
    elif name == "denormal_t":
        m[:3, 3] = np.array([0x00012345, 0x80000000, 0x80000001], np.uint32).view(F32)  # denormal, -0, -denormal
    elif name == "general":
        m = rng.normal(size=(4, 4)).astype(F32)
    elif name == "huge":
        m[:3, :3] = (m[:3, :3] * F32(1e30)).astype(F32)
    elif name == "reflect":
        m[:3, :3] = m[:3, :3][:, [1, 0, 2]]
    elif name == "tiny_scale":
        m[:3, :] = (m[:3, :] * F32(1e-30)).astype(F32)
    else:
        assert name == "rigid"
    return np.ascontiguousarray(m, F32)


def family_matrices(seed):
    rng = np.random.default_rng([seed, 99])
    return {name: matrix(name, rng) for name in FAMILIES}


def group_matrices(n_groups, seed, families=FAMILIES, rot=0):
    """one matrix per group, the families in turn (group g: families[(g + rot) % len])"""
    rng = np.random.default_rng([seed, n_groups, 17])
    pool = [matrix(name, rng) for name in families for _ in range(3)]
    pick = [(3 * ((g + rot) % len(families)) + int(rng.integers(3))) for g in range(n_groups)]
    return np.stack([pool[i] for i in pick]) if n_groups else np.zeros((0, 4, 4), F32)


def even_offsets(n, n_groups):
    """n records cut into n_groups near-equal groups (some empty when n < n_groups)"""
    return ((np.arange(n_groups + 1, dtype=np.int64) * n) // n_groups).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# group layouts

def group_layouts():
    """name -> offsets (int32, ascending from 0; the last one is the record count)"""
    rng = np.random.default_rng(404)
    L = {}
    L["single"] = [0, 300]
    L["one_two"] = np.concatenate([[0], np.cumsum([1, 2] * 70)])
    # sixty-four one-record groups filling one wave trip (records 64 .. 127), and again across a trip's end
    L["ones64"] = np.concatenate([[0, 64], 64 + np.arange(1, 65), [128 + 30], 158 + np.arange(1, 65), [300]])
    L["empty_edges"] = [0, 0, 0, 40, 40, 40, 40, 130, 131, 131, 200, 200, 200]
    L["seams"] = [0, 63, 64, 65, 255, 256, 257, 400]
    L["boundary"] = [0] + [256 * (d + 1) + d for d in range(65)] + [256 * 67]
    L["thousands"] = np.concatenate([[0], np.cumsum(rng.integers(0, 4, 3000))])
    return {k: np.asarray(v, np.int32) for k, v in L.items()}


SHAPES = ("size1", "size2", "ones64_in_trip", "empty_first", "empty_last", "empty_consecutive", "single", "thousands",
          "cut_255_256_257", "cut_63_64_65") + tuple("cut_d%d" % d for d in range(65))


def layout_shapes(off):
    """the group shapes a layout holds"""
    off = np.asarray(off, np.int64)
    size = np.diff(off)
    out = set()
    if (size == 1).any():
        out.add("size1")
    if (size == 2).any():
        out.add("size2")
    ones = size == 1
    for g in np.flatnonzero(ones):
        if off[g] % 64 == 0 and g + 64 <= len(size) and ones[g:g + 64].all():
            out.add("ones64_in_trip")
    if size[0] == 0:
        out.add("empty_first")
    if size[-1] == 0:
        out.add("empty_last")
    if ((size[:-1] == 0) & (size[1:] == 0)).any():
        out.add("empty_consecutive")
    if len(size) == 1:
        out.add("single")
    if len(size) >= 2048:
        out.add("thousands")
    cuts = set(off[1:-1].tolist())
    if {255, 256, 257} <= cuts:
        out.add("cut_255_256_257")
    if {63, 64, 65} <= cuts:
        out.add("cut_63_64_65")
    for d in range(65):
        if any(c >= 256 and (c - d) % 256 == 0 for c in cuts):
            out.add("cut_d%d" % d)
    return out


def changed_patterns(off):
    size = np.diff(np.asarray(off, np.int64))
    g = len(size)
    return {"all": np.ones(g, np.uint8), "none": np.zeros(g, np.uint8), "alternating": (np.arange(g) % 2).astype(np.uint8),
            "only_empty": (size == 0).astype(np.uint8)}


def layout_records(off, seed):
    """(records, class per record) for a layout: every class in every larger group"""
    return crafted_records(int(off[-1]), seed)


# ---------------------------------------------------------------------------------------------------------------------
# second trips

BIG_N = 600000
MARK_CAP = 2048 * 256       # k_mark_key's records per trip = one tail_hole_scan round of 8192 words
EXTRACT_TRIP = 64 * 256     # k_extract_marked's marked records per trip
RUN_KEY, LAST_WORD_KEY = 9, 11


def big_map(seed=600):
    """BIG_N records: finite coordinates (with a sprinkling of the special ones), every record live.  Keys: RUN_KEY for a run
    straddling record MARK_CAP, LAST_WORD_KEY inside the last 64-record word only, 3 elsewhere; ABSENT_KEY marks nothing, and
    big_map_all() marks everything."""
    rng = np.random.default_rng(seed)
    s = plain_records(rng, BIG_N, keys=(3,))
    pick = rng.random(BIG_N) < 0.01
    s["px"][pick] = rng.choice(SPECIALS[:7], int(pick.sum()))
    s["last_update"][MARK_CAP - 300:MARK_CAP + 300] = RUN_KEY
    last_word = (BIG_N - 1) // 64 * 64
    s["last_update"][last_word + 5:] = LAST_WORD_KEY
    return s


def big_map_all(s):
    a = s.copy()
    a["last_update"] = KEY
    return a


# ---------------------------------------------------------------------------------------------------------------------
# erase shapes

ERASE_SHAPES = ("tail_longer", "tail_equal", "tail_shorter", "tail_1", "hole_at_0", "hole_at_end", "n_0", "empty_store")


def erase_shape(store_n, begin, n):
    tail = store_n - (begin + n)
    out = set()
    if store_n == 0:
        out.add("empty_store")
    if n == 0:
        out.add("n_0")
        return out
    if begin == 0:
        out.add("hole_at_0")
    if tail == 0:
        out.add("hole_at_end")
    elif tail == 1:
        out.add("tail_1")
    if tail > n:
        out.add("tail_longer")
    elif tail == n:
        out.add("tail_equal")
    elif 0 < tail < n:
        out.add("tail_shorter")
    return out


# (segment sizes of the store, first and one-past-last segment to erase)
ERASE_CASES = (
    ((100, 50, 200), 1, 2), ((100, 200, 200), 1, 2), ((100, 200, 50), 1, 2), ((100, 200, 1), 1, 2), ((70, 300), 0, 1),
    ((70, 300), 1, 2), ((100, 0, 60), 1, 2), ((100, 60, 0), 2, 3), ((300, 17, 23, 500), 1, 3), ((64, 64), 0, 2), ((), 0, 0),
    ((1, 1, 1), 1, 2), ((257, 255, 256), 0, 1),
)


def segment_records(sizes, seed):
    """a map whose key-g records number sizes[g], interleaved; deactivating 0, 1, ... builds the store segment by segment"""
    rng = np.random.default_rng([seed, len(sizes)])
    n = int(sum(sizes))
    s, _ = crafted_records(n, seed)
    s["update_times"] = rng.integers(1, 9, n)
    s["last_update"] = rng.permutation(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)) if n else 0
    return s


# ---------------------------------------------------------------------------------------------------------------------
# schedules

OPS = ("map_upload", "map_warp", "map_extract", "map_append", "store_deactivate", "store_activate", "store_erase", "store_warp",
       "store_download")
SCHEDULE_SEEDS = (1, 2, 3, 4, 5, 6)
SCHEDULE_CAP = 9000
SCHEDULE_RECORDS, SCHEDULE_KEYS = 5000, 40


def schedule_records(rng, n, n_keys=SCHEDULE_KEYS):
    """mostly ordinary records under n_keys keys, one in eight of another class"""
    s = plain_records(rng, n, keys=np.arange(n_keys))
    cls = rng.integers(0, 8 * len(CLASSES), n)
    for c, name in enumerate(CLASSES):
        idx = np.flatnonzero(cls == c)
        s[idx] = class_records(rng, name, len(idx), key=int(rng.integers(n_keys)))
    return s


def make_schedule(seed, repeats=7):
    """[(operation, arguments...)], valid by construction: erases take unions of segments, warps tile the store with the
    segments' offsets, appends and activations stay within SCHEDULE_CAP.  Starts with a map_upload."""
    rng = np.random.default_rng([seed, 2024])
    model = StoreModel(SCHEDULE_CAP)
    ops, segs, parked = [], [], []

    def emit(*op):
        ops.append(op)
        return apply(model, op)

    emit("map_upload", schedule_records(rng, SCHEDULE_RECORDS))
    for name in rng.permutation(np.repeat(np.array(OPS + ("store_deactivate",)), repeats)):  # (twice the deactivations)
        name = str(name)
        if name in ("store_activate", "store_erase") and not segs:
            name = "store_deactivate"
        if name == "map_upload":
            emit("map_upload", schedule_records(rng, int(rng.integers(3000, SCHEDULE_RECORDS + 200))))
        elif name == "map_warp":
            emit("map_warp", matrix(str(rng.choice(FINITE_FAMILIES)), rng))
        elif name == "map_extract":
            parked.append(emit("map_extract", int(rng.integers(SCHEDULE_KEYS))))
        elif name == "map_append":
            s = parked.pop(int(rng.integers(len(parked)))) if parked else plain_records(rng, 37, keys=np.arange(SCHEDULE_KEYS))
            if len(model.map) + len(s) > SCHEDULE_CAP:
                emit("map_upload", schedule_records(rng, 3000))
            emit("map_append", s)
        elif name == "store_deactivate":
            b, n = emit("store_deactivate", int(rng.integers(SCHEDULE_KEYS)))
            segs.append([b, n])
        elif name == "store_activate":
            i = int(rng.integers(len(segs)))
            j = min(len(segs), i + int(rng.integers(1, 3)))
            b, n = segs[i][0], sum(x[1] for x in segs[i:j])
            if len(model.map) + n > SCHEDULE_CAP:
                emit("map_upload", schedule_records(rng, 3000))
            emit("store_activate", b, n)
        elif name == "store_erase":
            i = int(rng.integers(len(segs)))
            j = min(len(segs), i + int(rng.integers(1, 4)))
            b, n = segs[i][0], sum(x[1] for x in segs[i:j])
            emit("store_erase", b, n)
            del segs[i:j]
            for x in segs[i:]:
                x[0] -= n
        elif name == "store_warp":
            off = np.array([x[0] for x in segs] + [len(model.store)], np.int32) if segs else np.zeros(1, np.int32)
            g = len(off) - 1
            mats = np.stack([matrix(str(rng.choice(FINITE_FAMILIES)), rng) for _ in range(g)]) if g else np.zeros((0, 4, 4), F32)
            emit("store_warp", off, mats, (rng.random(g) < 0.6).astype(np.uint8))
        else:
            n_store = len(model.store)
            b = int(rng.integers(n_store + 1))
            emit("store_download", b, int(rng.integers(n_store - b + 1)))
    return ops


def apply(engine, op):
    """run one operation of a schedule on anything with StoreModel's methods (the model, the stand-in, the device)"""
    return getattr(engine, op[0])(*op[1:])


def check_schedule(ops, capacity=SCHEDULE_CAP):
    """the validity rules, checked on the model: returns {operation: count}, the erase shapes met, and the model at the end"""
    model = StoreModel(capacity)
    count = {name: 0 for name in OPS}
    bounds = [0]  # segment boundaries of the store
    shapes = set()
    for op in ops:
        name = op[0]
        count[name] += 1
        if name == "store_erase":
            b, n = op[1:]
            assert b in bounds and b + n in bounds, ("erase is no union of segments", op[1:], bounds)
            shapes |= erase_shape(len(model.store), b, n)
            bounds = sorted(set(x for x in bounds if x <= b) | set(x - n for x in bounds if x >= b + n))
        elif name == "store_warp":
            off = op[1]
            assert off[0] == 0 and (len(off) == 1 or off[-1] == len(model.store)) and (np.diff(off) >= 0).all(), "warp does not tile the store"
            assert set(off.tolist()) <= set(bounds)
        elif name == "store_activate":
            assert len(model.map) + op[2] <= capacity and op[1] + op[2] <= len(model.store)
        elif name == "map_append":
            assert len(model.map) + len(op[1]) <= capacity
        elif name == "store_download":
            assert op[1] + op[2] <= len(model.store)
        r = apply(model, op)
        if name == "store_deactivate":
            assert r[0] == bounds[-1]
            bounds.append(r[0] + r[1])
    return count, shapes, model


# ---------------------------------------------------------------------------------------------------------------------
# a schedule with real frames in between

def frames_schedule(frames, orc, model, dev=None):
    """Maintenance operations between fused frames: `frames` from synth.sequence, `orc` a PortOracle (its fuse_map is the
    reference for the frames), `model` a StoreModel; with `dev` (a FusionFunctions holding the frames in its slots, pipeline
    depth 12) every step also runs on the device -- single frames through fuse_frame_resident, runs of frames as one
    replay_enqueue chunk -- and map, store and cloud are compared after every step.  Returns what the census needs."""
    stats = {"shrunk": 0, "refilled": 0, "re_extracted": 0, "stale": 0, "steps": 0}
    rng = np.random.default_rng(77)
    t = [0]

    def check(tag):
        stats["steps"] += 1
        if dev is not None:
            same_state(dev, model, tag)

    def fuse(k, chunk):
        todo = list(range(t[0], t[0] + k))
        if dev is not None and chunk:
            dev.replay_enqueue(*dev.pack_replay(todo, [frames[i][4] for i in todo], np.stack([frames[i][3] for i in todo])))
        for i in todo:
            _, img, dep, pose, ref = frames[i]
            if dev is not None and not chunk:
                dev.fuse_frame_resident(i, ref, pose)
            holes, before = int((model.map["update_times"] == 0).sum()), len(model.map)
            after, n_new = orc.fuse_map(ref, img, dep, pose, model.map)
            stats["refilled"] += int(holes > 0 and n_new > 0)
            stats["shrunk"] += int(len(after) < before)
            model.map_set(after)
        t[0] += k
        check("frames to %d" % t[0])

    def op(*o):
        want = apply(model, o)
        if dev is not None:
            same_result(o[0], apply(dev, o), want)
        check(o)
        return want

    small = lambda: rigid(rng, 0.01)
    fuse(5, True)    # keyframe 0 (frames 0 .. 4)
    fuse(3, False)   # keyframe 1
    a = op("store_deactivate", 0)
    fuse(1, False)   # the holes are refilled, the rest closed by the compaction
    b = op("store_deactivate", 1)
    fuse(1, False)   # one more frame of keyframe 1: its surfels carry the key again
    again = op("map_extract", 1)
    stats["re_extracted"] = len(again)
    op("map_warp", small())
    fuse(2, True)    # ... and on to keyframe 2
    op("store_warp", np.array([0, a[1], a[1] + b[1]], np.int32), np.stack([small(), small()]), np.array([1, 1], np.uint8))
    stats["stale"] = int((_bits(model.cloud[:, :3]) != _bits(xyzi(model.store)[:, :3])).any(axis=1).sum())
    op("store_activate", *a)
    op("store_erase", *a)
    fuse(2, True)
    op("store_deactivate", 2)
    op("map_append", again)
    fuse(1, False)
    op("store_download", 0, len(model.store))
    stats["segments"] = (a[1], b[1])
    return stats


N_FRAMES = 15
