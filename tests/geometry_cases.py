"""Image sizes that stand against a constant of the frame kernels, and procedural frames for them.

The per-frame path (k_init_seeds -> three sweeps of k_assign / k_resolve / k_update_seeds* / k_commit_seeds -> k_pixel_normals /
k_seed_stats / k_seed_points -> k_seed_fit / k_seed_finish -> k_fuse_surfels -> k_frame_tail) is compared with the oracle at
many inputs elsewhere, but at ten image sizes.  dsm_create takes any size with 24 <= w, h <= 32767 and (w/8)(h/8) <= 65535;
GEOMETRIES below is the list of sizes at which a tile edge, a launch width, a label bit or a coordinate width of those kernels
is met for the first time.  No GPU and no reference sources are needed here: tests/test_cpu_geometry.py runs the census on the
oracle, tests/test_gpu_geometry.py the device against it.

  frames(geometry, n, variant) -> [(image, depth, pose, reference frame index)]   procedural, seeded, cheap at 4 megapixels
  census(geometry, records)    -> the conditions a replay by the oracle has to meet for the comparison to mean something
"""
import dataclasses

import numpy as np

from densesurfelmapping_amd.synth import Camera

CELL = 8
MAX_SEEDS = 65535
BIG_PIXELS = 500_000  # above: two frames per run instead of six
VARIANTS = 8


@dataclasses.dataclass(frozen=True)
class Geometry:
    w: int
    h: int
    against: str  # the constant this size stands against

    @property
    def gw(self):
        return self.w // CELL

    @property
    def gh(self):
        return self.h // CELL

    @property
    def S(self):
        return self.gw * self.gh

    @property
    def name(self):
        return f"{self.w}x{self.h}"

    @property
    def big(self):
        return self.w * self.h > BIG_PIXELS

    @property
    def n_frames(self):
        return 2 if self.big else 6

    @property
    def group_frames(self):
        """frames of the run that goes through a frame group of four: the group and a ragged end (the first n_frames of it are
        the run of the other forms)"""
        return 5 if self.big else 6

    @property
    def quiet_frame(self):
        """the frame with few grey levels: inside the first frame group of four, after the map exists"""
        return 1 if self.big else 2

    @property
    def camera(self):
        # fx != fy, the principal point off the centre and off the pixel grid; the focal length follows the longer side, so that
        # the widest ray of the 32767-pixel sides stays at tan 29 degrees
        f = 0.9 * max(self.w, self.h)
        return Camera(self.w, self.h, round(f, 3), round(1.07 * f, 3), round(0.47 * self.w + 0.25, 3), round(0.54 * self.h - 0.25, 3))


# small to large: the extreme sizes run last
GEOMETRIES = [
    Geometry(24, 24, "3x3 = 9 seeds: the smallest size dsm_create accepts; every seed a border seed; S < 16 (one k_init_seeds workgroup); S mod 4 = 1"),
    Geometry(28, 29, "3x3: residues 4 | 5, the `(size mod 8) > 4` rule's boundary on the y axis"),
    Geometry(29, 28, "3x3: residues 5 | 4, the same boundary on the x axis"),
    Geometry(31, 31, "3x3: residue 7 on both axes on the smallest grid, 177 of 961 pixels without a candidate cell"),
    Geometry(50, 43, "6x5 = 30 seeds: S mod 4 = 2 (the partial last group of k_seed_fit)"),
    Geometry(63, 27, "7x3 = 21 seeds: w = pitch - 1, gh = 3"),
    Geometry(64, 32, "8x4 = 32 seeds: w = pitch = one tile column; S < 64 (half a lane-form wave)"),
    Geometry(65, 33, "8x4 = 32 seeds: a tile column of one pixel; h = 1 mod 4 and mod 16 (a tile row of one pixel row)"),
    Geometry(72, 56, "9x7 = 63 seeds: one lane-form wave less one; S mod 4 = 3"),
    Geometry(64, 64, "8x8 = 64 seeds: one lane-form wave exactly"),
    Geometry(104, 40, "13x5 = 65 seeds: one lane-form wave and one seed"),
    Geometry(129, 81, "16x10 = 160 seeds: w = 64k + 1 over more than one tile column, h = 1 mod 16 over more than one tile row"),
    Geometry(136, 120, "17x15 = 255 seeds: g_seed_thr's workgroup of 256 less one"),
    Geometry(128, 128, "16x16 = 256 seeds: that workgroup exactly; w = 64k"),
    Geometry(160, 104, "20x13 = 260 seeds: beyond it"),
    Geometry(520, 24, "65x3 = 195 seeds: gh = 3 over many tile columns; S mod 4 = 3"),
    Geometry(24, 520, "3x65 = 195 seeds: gw = 3 (seed_cell's smallest divisor) over many tile rows"),
    Geometry(32767, 24, "4095x3 = 12285 seeds: the largest width: pitch 32768, x to 32766, 512 tile columns, residue 7"),
    Geometry(24, 32767, "3x4095 = 12285 seeds: the largest height: y to 32766 (bit 30 of x | y << 16), 8192 tile rows, residue 7"),
    Geometry(2048, 1032, "256x129 = 33024 seeds: the cheapest size with labels >= 32768 (bit 15 of a label_t)"),
    Geometry(2040, 2056, "255x257 = 65535 seeds: kMaxSeeds exactly; the top label 65534 beside kNoLabel"),
]
BY_NAME = {g.name: g for g in GEOMETRIES}
assert len(BY_NAME) == len(GEOMETRIES)
assert all(24 <= g.w <= 32767 and 24 <= g.h <= 32767 and g.S <= MAX_SEEDS for g in GEOMETRIES)
assert [g.w * g.h for g in GEOMETRIES[-4:]] == sorted(g.w * g.h for g in GEOMETRIES)[-4:] and sum(g.big for g in GEOMETRIES) == 4


# ------------------------------------------------------------------------------------------------------------ frames
def pose_of(t, variant):
    """the camera a few millimetres further per frame, every variant in its own direction"""
    p = np.eye(4, dtype=np.float32)
    sx, sy = (1, -1)[variant & 1], (1, -1)[(variant >> 1) & 1]
    p[:3, 3] = np.array([0.004 * sx, 0.002 * sy, 0.003 + 0.0005 * variant], np.float32) * t
    return p


def _depth(g, t, variant):
    """Three planes of one world seen from pose_of(t, variant): a wall square to the camera (left half), a slanted plane (upper
    right) and a nearer one slanted the other way (lower right) -- step edges where they meet."""
    cam = g.camera
    u = (np.arange(g.w, dtype=np.float64) - cam.cx) / cam.fx
    v = (np.arange(g.h, dtype=np.float64) - cam.cy) / cam.fy
    rx, ry = np.meshgrid(u, v)
    c = pose_of(t, variant)[:3, 3].astype(np.float64)
    planes = [((0.0, 0.0, 1.0), 4.0), ((0.30, 0.10, 1.0), 3.0), ((-0.25, 0.20, 1.0), 2.2)]
    z = [(d - (n[0] * c[0] + n[1] * c[1] + n[2] * c[2])) / (n[0] * rx + n[1] * ry + n[2]) for n, d in planes]
    fx = np.arange(g.w)[None, :] * 2 >= g.w
    fy = np.arange(g.h)[:, None] * 20 >= g.h * 11
    return np.where(~fx, z[0], np.where(~fy, z[1], z[2])).astype(np.float32)


def frames(g, n=None, variant=0):
    """n frames (g.n_frames if None) of run `variant` (0..7: eight distinguishable runs for the handles of a batch).
    Grey blocks of 11 x 9 pixels with a ramp and a little noise over them, so that superpixels leave their cells; depth: the three
    planes with 0.1 % noise, 1.5 % zero holes and a few +inf and NaN pixels.  Frame g.quiet_frame has two grey levels and the planes
    alone: few candidates differ in cost, seeds stop moving and k_resolve has pixels to decide."""
    assert 0 <= variant < VARIANTS
    n = g.n_frames if n is None else n
    x, y = np.arange(g.w)[None, :], np.arange(g.h)[:, None]
    out = []
    for t in range(n):
        rng = np.random.default_rng(7919 * (g.w * 40000 + g.h) + 64 * variant + t)
        dep = _depth(g, t, variant)
        if t == g.quiet_frame:
            img = np.where(((x + 3 * variant) // 24 + (y + 2 * variant) // 16) % 2, 64, 192).astype(np.uint8)
        else:
            img = (((x + 3 * variant) // 11 + 2 * ((y + variant) // 9)) * 53 % 160 + 40 + (3 * x + 5 * y) % 17
                   + rng.integers(0, 6, (g.h, g.w))).astype(np.uint8)
            r = rng.random((g.h, g.w), dtype=np.float32)
            dep = dep * (1.0 + 0.001 * (rng.random((g.h, g.w), dtype=np.float32) - 0.5))
            dep = np.where(r < 0.015, 0.0, dep).astype(np.float32)
            # a few pixels of what a publisher hands over besides metres, two of each at least: one in 5000 pixels +inf (an unmatched
            # disparity) and as many NaN.  Few: a +inf among a superpixel's depths makes its robust mean +inf and the seed fits no plane
            few = rng.choice(g.w * g.h, 2 * max(2, g.w * g.h // 5000), replace=False)
            dep.reshape(-1)[few[::2]] = np.inf
            dep.reshape(-1)[few[1::2]] = np.nan
        out.append((img, np.ascontiguousarray(dep, np.float32), pose_of(t, variant), t // 3))
    return out


# ------------------------------------------------------------------------------------------------------------ census
def unlabelled_pixels(g):
    """pixels beyond every cell's reach (the `(size mod 8) > 4` rule): h * max(0, w - 8 gw - 4) + w * max(0, h - 8 gh - 4) less
    the corner counted twice"""
    ex, ey = max(0, g.w - CELL * g.gw - 4), max(0, g.h - CELL * g.gh - 4)
    return g.h * ex + g.w * ey - ex * ey


def census(g, records):
    """records[t] = (new count, labels, seeds, map) after frame t of a replay by an oracle; asserts the conditions under which a
    comparison at this size has compared what the size is for, and returns the figures."""
    assert len(records) >= 2
    out = {"unlabelled": unlabelled_pixels(g)}
    for t, (k, lab, seeds, local) in enumerate(records):
        assert lab.shape == (g.h, g.w) and len(seeds) == g.S
        assert int((lab < 0).sum()) == out["unlabelled"], (g.name, t, int((lab < 0).sum()), out["unlabelled"])
        assert lab.max() < g.S and lab.min() >= -1
    lab0 = records[0][1]
    owners = np.bincount(lab0[lab0 >= 0], minlength=g.S)
    assert (owners > 0).all(), f"{g.name}: seeds {np.flatnonzero(owners == 0)[:5]} own no pixel after frame 0"
    out["top_label"] = int(lab0.max())
    if g.S > 32768:
        assert (lab0 >= 32768).any(), f"{g.name}: no label sets bit 15"
    assert out["top_label"] == g.S - 1
    final = records[-1][3]
    out["surfels"] = len(final)
    out["fused_again"] = int((final["update_times"] >= 2).sum())
    assert out["surfels"] > 0 and out["fused_again"] > 0, (g.name, out)
    if g.S >= 64:
        assert out["surfels"] >= g.S // 4, (g.name, out)
    out["stable_after_quiet"] = int(records[g.quiet_frame][2]["stable"].astype(bool).sum())
    assert out["stable_after_quiet"] > 0, f"{g.name}: the quiet frame leaves no seed stable"
    return out
