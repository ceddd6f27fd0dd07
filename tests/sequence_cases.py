"""Shared by tests/test_cpu_sequence_cases.py and tests/test_gpu_sequence_walk.py: the inputs that drive the ONE walk of the surfel
sequence (csrc/dsm_k_sequence.h) through all four products -- cloud, mesh, render, grid -- at its edge sizes, pass patterns and
run layouts, with every expected value from numpy and the host checkers of render_cases.py / grid_cases.py.

Every record owns a slot: map record i the slot i, store record s the slot SLOTS - 1 - s.  A slot is one pixel of CAM (for the
records of `render_placed`) or one voxel of GRID (`grid_placed`), and the record is a tiny surfel in the middle of it.  So every
member of a sequence shows in the index plane on its own -- as long as no run list names a store record twice -- and a shifted,
dropped or doubled sequence number changes the plane.  `expected_index` asserts exactly that before it hands the plane out."""
import numpy as np

import grid_cases as gc
import render_cases as rc

T = 1024                     # api.CLOUD_TILE (asserted by the GPU test): records per workgroup of the walk
CAM = rc.CAM_96              # 96 x 64 pixels
GRID = gc.spec((-12.0, -1.0, -1.0), 0.25, (96, 8, 8))
SLOTS = 96 * 64              # of the image and of the grid alike
STORE_N = 130                # store records; the largest map has 5 T + 3
SELECT = 1                   # mature: update_times >= 5
assert CAM.width * CAM.height == SLOTS == GRID.nx * GRID.ny * GRID.nz and 5 * T + 3 + STORE_N <= SLOTS

MAP_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17)
N_PATTERN = 5 * T + 3
FRONT = [(3, 65)]            # the run in front of the pattern maps: base > 0, not a multiple of 64


def _patterns():
    i = np.arange(N_PATTERN)
    wave = np.full(N_PATTERN, 7)
    wave[T + 256:T + 512] = 4          # wave 1 of tile 1: all of its four chunks
    tile = np.full(N_PATTERN, 7)
    tile[2 * T:3 * T] = 0
    return {"none pass": np.zeros(N_PATTERN, int), "all pass": np.full(N_PATTERN, 7), "alternating": np.where(i % 2 == 0, 5, 4),
            "every 64th": np.where(i % 64 == 63, 9, 0), "one wave failing": wave, "one tile failing": tile}


PATTERNS = _patterns()

# run lists in front of a map part of N_BEHIND records: total lengths 0, 1, 63, 64, 65; no store record twice
N_BEHIND = T + 65
RUNS = {
    "no runs": [],
    "empty runs only": [(5, 0), (9, 0)],
    "one run of 1": [(7, 1)],
    "one run of 63": [(10, 63)],
    "one run of 64": [(10, 64)],
    "one run of 65": [(10, 65)],
    "63 runs of 1": [(2 * k + 1, 1) for k in range(63)],
    "64 runs of 1, descending": [(128 - 2 * k, 1) for k in range(64)],
    "65 runs of 1": [(2 * k, 1) for k in range(65)],
    "empty runs in between, 63": [(0, 0), (3, 20), (50, 0), (40, 0), (60, 43), (0, 0)],
    "a boundary inside a wave, 64": [(64, 1), (0, 63)],
    "a boundary inside a wave, 65": [(100, 30), (0, 35)],
}


def ut_random(n, seed):
    """update_times about the threshold of SELECT, a little over half passing"""
    return np.random.default_rng(seed).choice(np.array([0, 4, 5, 7, 9, -3]), n)


def cases():
    """[(name, update_times of the map, run list)]"""
    out = [("n=%d" % n, ut_random(n, 100 + n), []) for n in MAP_SIZES]
    out += [(name, ut, FRONT) for name, ut in PATTERNS.items()]
    out += [(name, ut_random(N_BEHIND, 7), segs) for name, segs in RUNS.items()]
    return out


def run_total(segs):
    return sum(c for _, c in segs)


def _slots_of(n, store):
    return SLOTS - 1 - np.arange(n) if store else np.arange(n)


def render_placed(surfel_dtype, ut, store=False):
    """a record per entry of ut, each facing the camera at the identity pose in the middle of its own pixel"""
    slot = _slots_of(len(ut), store)
    a = np.zeros(len(ut), surfel_dtype)
    u, v, z = slot % CAM.width, slot // CAM.width, 2.0
    a["px"], a["py"], a["pz"] = (u - CAM.cx) / CAM.fx * z, (v - CAM.cy) / CAM.fy * z, z
    a["nz"] = -1.0
    a["size"] = 0.004             # a pixel is z / fx = 0.024 wide
    a["color"] = slot % 251
    a["weight"] = 1.0
    a["update_times"] = ut
    return a


def grid_placed(surfel_dtype, ut, store=False):
    """a record per entry of ut, each at the centre of its own voxel"""
    slot = _slots_of(len(ut), store)
    a = np.zeros(len(ut), surfel_dtype)
    x, y, z = slot % GRID.nx, slot // GRID.nx % GRID.ny, slot // (GRID.nx * GRID.ny)
    a["px"], a["py"], a["pz"] = gc.centres(GRID, 0)[x], gc.centres(GRID, 1)[y], gc.centres(GRID, 2)[z]
    a["nz"] = 1.0
    a["size"] = 0.1 * GRID.voxel
    a["color"] = slot % 251
    a["weight"] = 1.0
    a["update_times"] = ut
    return a


def store_records(surfel_dtype, place):
    """the STORE_N records of the store (they all leave a map with store_deactivate(0): last_update 0)"""
    return place(surfel_dtype, np.full(STORE_N, 7), store=True)


def passing(m):
    return m[m["update_times"] >= 5]


def sequence(store, m, segs):
    """the runs FIRST, then the map part (the mesh, the render, the grid; the cloud has the map part first)"""
    return np.concatenate([store[b:b + c] for b, c in segs] + [passing(m)])


PLACE = {"render": render_placed, "grid": grid_placed}


def expected(product, seq):
    """every output of the product for the sequence from its brute-force host checker; every member is in the index plane"""
    exp = rc.host_render(seq, CAM, rc.IDENTITY) if product == "render" else gc.host_all(seq, GRID)
    shown = np.unique(exp["index"][exp["index"] >= 0])
    assert len(shown) == len(seq), (product, len(shown), len(seq))
    return exp
