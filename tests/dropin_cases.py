"""Large maps for the drop-in calls' delta download (dsm_fuse_map / dsm_fuse_initialize_map on the caller's own array): short
sequences of calls with caller edits in between, at the sizes where the path branches -- k_frame_tail's one-workgroup limit
(kTailFastWords * 64 = 262 144 surfels), its hole chunks (kTailChunkWords * 64 = 524 288), the doublings of the page-locked
shadow (65 536 records first), the 60 % rule that sends a call to the full download, the first transfer's `guess`, and the
1 MiB chunks of the host compare (kParChunk).

Built from numpy and the ORACLE alone (oracle/bindings.py, PortOracle), never from the product, with counter-based hashes
and seeded default_rng only.  Camera: synth.TINY (160x96, 240 seeds): a frame of its own changes a handful of 64-record
groups, so the builder decides which groups change.  A map is made of

  * parked records (test_gpu_adversarial._parked): live, far behind the camera, never touched;
  * visible records: the oracle's map after three frames of synth.sequence(TINY, Scene()), placed at chosen indices;
  * stale records: last_update = -100, update_times 1..4 -- pruned by the next frame wherever they sit (FF.cpp:206-210);
  * dead records: update_times = 0 on entry.

A case is a list of Steps.  A Step holds the caller's edits since the previous call (OPS below, applied with apply_edits to
the caller's buffer and mirrored in the builder's model of it), the frame, and what the oracle made of the edited map: sizes,
the new-surfel count, the touched set T and the records of T's groups (`rec_idx`, `recs`: model[rec_idx] = recs turns the
edited input into the expected output -- everything outside T is equal by T's definition, so a case keeps a few kilobytes per
call instead of two 23 MB maps).

T, from the oracle's input and output alone: the groups that hold a record whose bytes differ between input and output below
min(n_in, n_out), and the groups of the records [n_in, n_out) a growing call appends.  (Read literally, "every group from
min(n_in, n_out) // 64 up to the output's last group" also names the output's last, partly filled group of a call that does
NOT grow the map, where no record need differ: with it |T| could not be 0 for a call that changes nothing, and
last_groups >= |T| would not follow from parity.  For a growing call the two readings are the same set.)

With 240 seeds a TINY frame creates 35-55 surfels (K), so the chunk_seam variants with K == k and K > k hold K, respectively
a dozen, holes in all -- in both hole chunks and on both sides of index 524 288 -- and only the K < k variant the few hundred
per chunk.
"""
import dataclasses
import time

import numpy as np

from densesurfelmapping_amd import synth
from oracle import bindings as ob
from test_gpu_adversarial import _parked

CAM = synth.TINY
S = (CAM.width // 8) * (CAM.height // 8)  # 240 seeds: dropin_reserve asks for n_in + S records of shadow
GROUP = 64
TAIL_FAST = 4096 * 64          # kTailFastWords * 64 (dsm_device.h)
HOLE_CHUNK = 8192 * 64         # kTailChunkWords * 64
SHADOW_FIRST = 1 << 16         # the shadow's first size (dropin_reserve), doubled from there
PAR_CHUNK = 1 << 20            # kParChunk: bytes per task of the host compare
CAPACITY = 1 << 20             # records of the caller's buffer and of the handle
REC = ob.SURFEL_DTYPE.itemsize
GUARD_BYTE = 0xA5

_FRAMES = None
_VISIBLE = None
ORACLE_SECONDS = [0.0]  # the oracle's share of everything built so far


def frames():
    """frames 0..13 of the TINY scene (t, image, depth, pose, ref_idx); ref_idx <= 2, so that nothing a call creates goes stale"""
    global _FRAMES
    if _FRAMES is None:
        _FRAMES = list(synth.sequence(CAM, synth.Scene(), 14))
    return _FRAMES


def visible():
    global _VISIBLE
    if _VISIBLE is None:
        orc = ob.PortOracle(CAM)
        lo = np.zeros(0, ob.SURFEL_DTYPE)
        for t, img, dep, pose, ref in frames()[:3]:
            lo, _ = orc.fuse_map(ref, img, dep, pose, lo)
        _VISIBLE = lo
    return _VISIBLE


def blind_frame():
    """all-+inf depth from a pose a kilometre down the road: no surfel is in view (none deleted), no superpixel creates one"""
    t, img, dep, pose, ref = frames()[3]
    far = pose.copy()
    far[2, 3] += 1000.0
    return (t, img, np.full_like(dep, np.inf), far, ref)


def guard_buffer(dtype=ob.SURFEL_DTYPE):
    return np.full(CAPACITY * REC, GUARD_BYTE, np.uint8).view(dtype)


def raw(a):
    """records as rows of bytes"""
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), REC)


# ---- the caller's edits.  OPS:
#   ("parked", start, count, seed)   count parked records written from `start` (the caller appends re-activated keyframes)
#   ("scatter", idx, recs)           records written at the indices idx
#   ("size", n)                      the caller's array now has n records (truncation, or the end of an append)
#   ("byte", offset, xor)            one byte of the array, through its uint8 view
def apply_edits(arr, n, ops):
    for op in ops:
        if op[0] == "parked":
            arr[op[1]:op[1] + op[2]] = _parked(ob, op[2], op[3]).astype(arr.dtype)
        elif op[0] == "scatter":
            arr[op[1]] = op[2].astype(arr.dtype)
        elif op[0] == "size":
            n = op[1]
        elif op[0] == "byte":
            arr.view(np.uint8)[op[1]] ^= op[2]
        else:
            raise ValueError(op[0])
    return n


def touched(a_in, out):
    n_in, n_out = len(a_in), len(out)
    lo = min(n_in, n_out)
    diff = np.flatnonzero((raw(a_in[:lo]) != raw(out[:lo])).any(axis=1)) // GROUP
    grown = np.arange(n_in // GROUP, (n_out + GROUP - 1) // GROUP) if n_out > n_in else np.zeros(0, np.int64)
    return np.union1d(diff, grown).astype(np.int64)


def is_hole_on_entry(a, ref):
    """dead, or stale by FF.cpp:206-210 (pruned before anything else is looked at)"""
    return (a["update_times"] == 0) | ((ref - a["last_update"] > 5) & (a["update_times"] < 5))


@dataclasses.dataclass
class Step:
    kind: str            # "fuse_map" | "init_map" | "resident"
    edits: list          # the caller's edits before this call
    frame: tuple         # (t, image, depth, pose, ref_idx)
    expect: str = "delta"  # "delta" | "full": the download this call is built for
    label: str = ""
    n_in: int = 0
    n_out: int = 0
    k_new: int = 0
    T: np.ndarray = None
    rec_idx: np.ndarray = None
    recs: np.ndarray = None
    new: np.ndarray = None        # init_map: the new surfels, handed back separately
    census: dict = dataclasses.field(default_factory=dict)
    foreign_edits: list = None    # resident: edits of a COPY of the caller's state that goes up before the resident frame

    @property
    def groups_out(self):
        return (self.n_out + GROUP - 1) // GROUP

    @property
    def ratio(self):
        return len(self.T) / max(self.groups_out, 1)


class Run:
    """the builder's model of the caller's buffer and the oracle behind it"""

    def __init__(self):
        self.orc = ob.PortOracle(CAM)
        self.model = guard_buffer()
        self.n = 0
        self.pending = []
        self.steps = []
        self.calls = 0

    # ---- edits
    def edit(self, *ops):
        self.n = apply_edits(self.model, self.n, ops)
        self.pending += ops

    def reset(self, n, seed):
        self.edit(("parked", 0, n, seed), ("size", n))

    def resize(self, n, seed):
        """truncate, or append parked records, to n records"""
        if n > self.n:
            self.edit(("parked", self.n, n - self.n, seed))
        self.edit(("size", n))

    def put_visible(self, at):
        v = visible()[:max(0, min(len(visible()), self.n - at))]
        self.edit(("scatter", np.arange(at, at + len(v)), v.copy()))

    def mark(self, idx, kind):
        idx = np.unique(np.asarray(idx, np.int64))
        idx = idx[(idx >= 0) & (idx < self.n)]
        r = self.model[idx].copy()
        if kind == "stale":
            r["last_update"] = -100
            r["update_times"] = 1 + (synth._uniform01(idx.astype(np.uint32), 8) * 4).astype(np.int32)
        else:
            r["update_times"] = 0
        self.edit(("scatter", idx, r))
        return idx

    def stale_one_per_group(self, groups, salt):
        groups = np.asarray(groups, np.int64)
        off = (synth._uniform01(groups.astype(np.uint32), salt) * GROUP).astype(np.int64)
        return self.mark(groups * GROUP + off, "stale")

    # ---- calls
    def next_frame(self):
        return frames()[3 + self.calls % 11]

    def _timed(self, f, *a):
        t0 = time.perf_counter()
        out = f(*a)
        ORACLE_SECONDS[0] += time.perf_counter() - t0
        return out

    def probe(self, frame=None):
        """(K, k) of the next call on the map as it stands, nothing recorded"""
        t, img, dep, pose, ref = frame or self.next_frame()
        out, k_new = self._timed(self.orc.fuse_map, ref, img, dep, pose, self.model[:self.n])
        return k_new, self.n + k_new - len(out)

    def _census(self, a_in, ref, n_out, k_new):
        holes = np.flatnonzero(is_hole_on_entry(a_in, ref))
        return {"K": k_new, "k": len(a_in) + k_new - n_out,  # n_out = n_in + K - k (SM.cpp:1087-1109)
                "entry_holes_by_chunk": np.bincount(holes // HOLE_CHUNK, minlength=len(a_in) // HOLE_CHUNK + 1).tolist(),
                "entry_holes": holes,
                # records in front of the camera (parked ones sit at z <= -50): the visible block and what earlier calls created
                "entry_in_front": np.flatnonzero((a_in["pz"] > -40.0) & ~is_hole_on_entry(a_in, ref))}

    def fuse(self, label="", expect="delta", frame=None):
        fr = frame or self.next_frame()
        t, img, dep, pose, ref = fr
        a_in = self.model[:self.n].copy()
        out, k_new = self._timed(self.orc.fuse_map, ref, img, dep, pose, a_in)
        st = Step("fuse_map", self.pending, fr, expect, label, len(a_in), len(out), k_new)
        st.T = touched(a_in, out)
        st.census = self._census(a_in, ref, len(out), k_new)
        # K < k: a hole of the first hole chunk that now holds a record the input had behind the output's end (a move from the
        # end of the array: SM.cpp:1096-1109)
        c = st.census
        if c["K"] < c["k"] and len(a_in) > HOLE_CHUNK:
            tail = {r.tobytes() for r in raw(a_in[len(out):])}
            low = c["entry_holes"][c["entry_holes"] < min(HOLE_CHUNK, len(out))]
            c["moves_into_chunk0"] = int(sum(raw(out[i:i + 1])[0].tobytes() in tail for i in low))
            c["sources_from"] = len(out)
        self._commit(st, out)
        return st

    def init_map(self, label=""):
        """dsm_fuse_initialize_map, then the caller's own refill / append loop (SM.cpp:1077-1109 -- the oracle's fuse_map IS
        that loop) as edits in front of the next call"""
        fr = self.next_frame()
        t, img, dep, pose, ref = fr
        a_in = self.model[:self.n].copy()
        out, new = self._timed(self.orc.fuse_initialize_map, ref, img, dep, pose, a_in)
        final, k_new = self._timed(self.orc.fuse_map, ref, img, dep, pose, a_in)
        assert k_new == len(new)
        st = Step("init_map", self.pending, fr, "delta", label, len(a_in), len(out), len(new), new=new)
        st.T = touched(a_in, out)
        st.census = self._census(a_in, ref, len(final), k_new)
        self._commit(st, out)
        lo = min(len(out), len(final))
        idx = np.concatenate([np.flatnonzero((raw(out[:lo]) != raw(final[:lo])).any(axis=1)), np.arange(lo, len(final))])
        self.edit(("scatter", idx, final[idx].copy()), ("size", len(final)))
        return st

    def resident(self, foreign_groups, salt, label=""):
        """a resident frame on a map of its own (the caller's state with stale records in `foreign_groups`), which leaves flags
        behind; then the caller's state goes back up.  The caller's array does not change."""
        assert not self.pending
        fr = self.next_frame()
        t, img, dep, pose, ref = fr
        keep_model, keep_n = self.model[:self.n].copy(), self.n
        self.stale_one_per_group(foreign_groups, salt)
        foreign, self.pending = self.pending, []
        a_in = self.model[:self.n].copy()
        out, _ = self._timed(self.orc.fuse_map, ref, img, dep, pose, a_in)
        st = Step("resident", [], fr, "none", label, keep_n, keep_n, 0, foreign_edits=foreign)
        st.T = np.zeros(0, np.int64)
        st.census = {"foreign_T": touched(a_in, out)}
        self.model[:keep_n] = keep_model
        self.n = keep_n
        self.steps.append(st)
        self.calls += 1
        return st

    def _commit(self, st, out):
        g = st.T
        idx = (g[:, None] * GROUP + np.arange(GROUP)[None, :]).ravel()
        st.rec_idx = idx[idx < len(out)]
        st.recs = out[st.rec_idx].copy()
        self.model[st.rec_idx] = st.recs
        self.n = len(out)
        assert np.array_equal(raw(self.model[:self.n]), raw(out)), "T does not cover what the oracle changed"
        self.pending = []
        self.steps.append(st)
        self.calls += 1


def spread_groups(n_groups, count, salt):
    """`count` distinct groups of the first n_groups, hash-chosen"""
    order = np.argsort(synth._uniform01(np.arange(n_groups, dtype=np.uint32), salt), kind="stable")
    return np.sort(order[:count])


# ---------------------------------------------------------------------------------------------------------------------
# the chunk_seam maps (also under initialize_map_large, foreign_flags_large and capacity_then_recover)

CHUNK_SEAM_N = 530_048  # 8282 groups: the old end on a group boundary; two hole chunks


def chunk_seam_map(run, variant, seed=21):
    n = CHUNK_SEAM_N - (48 if variant == "K<k" else 0)
    run.reset(n, seed)
    run.put_visible(HOLE_CHUNK - 40)       # the visible block straddles index 524 288 ...
    run.mark([HOLE_CHUNK - 1], "stale")    # ... with a stale record on one side of it
    run.mark([HOLE_CHUNK], "dead")         # ... and a dead one on the other
    rng = np.random.default_rng(seed)
    if variant == "K<k":  # a few hundred holes per chunk, a hundred of them among the records the move chain takes from the end
        run.mark(rng.choice(np.arange(GROUP, HOLE_CHUNK - 200), 300, replace=False), "stale")
        run.mark(rng.choice(np.arange(HOLE_CHUNK + 200, n - 500), 150, replace=False), "stale")
        run.mark(rng.choice(np.arange(n - 400, n), 100, replace=False), "dead")
        run.mark(rng.choice(np.arange(HOLE_CHUNK + 200, n - 500), 50, replace=False), "dead")
        return
    run.mark(rng.choice(np.arange(GROUP, HOLE_CHUNK - 200), 5, replace=False), "stale")
    run.mark(rng.choice(np.arange(HOLE_CHUNK + 200, n - 500), 5, replace=False), "dead")
    if variant == "K==k":
        K, k = run.probe()
        assert 0 < k < K, (K, k)
        more = K - k  # (stale records are pruned before they can fuse: K stays)
        cand = np.stack([70_001 + 640 * np.arange(more), HOLE_CHUNK + 2001 + 64 * np.arange(more)], 1).ravel()  # chunk 0, 1, 0, 1 ...
        cand = cand[~is_hole_on_entry(run.model[cand], run.next_frame()[4])]
        run.mark(cand[:more], "stale")
        K2, k2 = run.probe()
        assert K2 == k2 == K, (K, K2, k2)


def _seam_262144(run):
    for i, n0 in enumerate((TAIL_FAST - 1, TAIL_FAST, TAIL_FAST + 1)):
        run.reset(n0, 11 + i)
        run.put_visible(TAIL_FAST - 40)
        run.mark([0, 63, 64, TAIL_FAST - 1, TAIL_FAST, n0 - 3, n0 - 70], "stale")
        run.fuse(f"entry {n0}")
    # the caller appends and truncates: above the limit, far below it (the large tail on a small map), just below it so that
    # the frame itself carries the map across, above it without an edit, and back
    run.resize(200_000, 31)
    run.fuse("truncated to 200 000")
    run.resize(TAIL_FAST - 60, 32)
    run.fuse("appended to 262 084")
    run.resize(300_000, 33)
    run.put_visible(TAIL_FAST - 40)  # (live on both sides of the limit this time: the entry maps end there)
    run.fuse("appended to 300 000")
    run.resize(TAIL_FAST - 20, 34)
    run.mark([5], "dead")
    run.fuse("truncated to 262 124: the frame crosses")
    run.fuse("no edit, above")
    run.resize(TAIL_FAST - 1000, 35)
    run.fuse("truncated below again")


def _chunk_seam(run):
    chunk_seam_map(run, "K<k")
    run.fuse("K<k")
    chunk_seam_map(run, "K>k")
    run.fuse("K>k, old end on a group boundary")
    run.mark([100, HOLE_CHUNK - 2, HOLE_CHUNK + 1, HOLE_CHUNK + 5000], "dead")
    run.fuse("K>k, old end inside a group")
    chunk_seam_map(run, "K==k")
    run.fuse("K==k")


def _shadow_growth(run):
    run.reset(SHADOW_FIRST - S, 41)
    run.put_visible(1000)
    for j, thr in enumerate((SHADOW_FIRST, 2 * SHADOW_FIRST, 4 * SHADOW_FIRST, 8 * SHADOW_FIRST)):
        run.resize(thr - S, 42 + 3 * j)
        run.fuse(f"n_in + {S} = {thr}: the last call that fits")
        run.resize(thr - S + 1, 43 + 3 * j)
        run.fuse(f"n_in + {S} = {thr + 1}: the shadow is regrown")
        run.stale_one_per_group(spread_groups(run.n // GROUP, 150, 60 + j), 70 + j)
        run.fuse("150 groups against the new buffers")


def _margin_groups(run, frac):
    """stale records, one per group, so that |T| is about `frac` of the OUTPUT's groups: the call shrinks the map by a record
    per hole, |T| ~ G, so G = frac * (n - G) / 64"""
    n = run.n
    g = int(frac * n / GROUP / (1.0 + frac / GROUP))
    return spread_groups(int(0.9 * (n // GROUP)), g, 80)  # (below the new end: every one of them is in the output)


def _fallback_margin(run):
    run.reset(300_000, 51)
    run.put_visible(TAIL_FAST - 40)
    run.stale_one_per_group(_margin_groups(run, 0.545), 81)
    run.fuse("0.55 of the groups")
    run.fuse("after the 0.55 call")
    run.stale_one_per_group(_margin_groups(run, 0.655), 82)
    run.fuse("0.65 of the groups", expect="full")
    run.fuse("the first delta call after a full download")


def _guess_series(run):
    run.reset(280_000, 61)
    run.put_visible(TAIL_FAST - 40)
    run.fuse("tiny")
    run.stale_one_per_group(spread_groups(run.n // GROUP, 400, 90), 91)
    run.fuse("large: a second transfer")
    run.fuse("tiny: an oversized first transfer")
    run.fuse("zero", frame=blind_frame())
    run.stale_one_per_group(spread_groups(run.n // GROUP, 400, 92), 93)
    run.fuse("large: a second transfer from guess = 8")


def _initialize_map_large(run):
    chunk_seam_map(run, "K<k")
    run.init_map("fuse_initialize_map, K<k map")
    run.fuse("fuse_map on what the caller made of it")
    run.init_map("fuse_initialize_map again")
    run.fuse("fuse_map again")


def _foreign_flags_large(run):
    chunk_seam_map(run, "K>k")
    run.fuse("before")
    groups = np.concatenate([spread_groups(HOLE_CHUNK // GROUP, 300, 94), HOLE_CHUNK // GROUP + spread_groups(80, 60, 95)])
    run.resident(groups, 96, "resident frame, flags in both chunks")
    run.fuse("after: the foreign flags are cleared")


def _caller_edits(run):
    run.reset(300_000, 71)
    run.put_visible(TAIL_FAST - 40)
    run.fuse("first call")
    seams = lambda: [PAR_CHUNK * i for i in range(1, run.n * REC // PAR_CHUNK + 1) if PAR_CHUNK * i < run.n * REC]
    picks = [("first byte", lambda: 0), ("last byte", lambda: run.n * REC - 1)]
    for name, which in (("first", 0), ("middle", None), ("last", -1)):
        seam = (lambda w=which: seams()[len(seams()) // 2 if w is None else w])
        picks.append((f"before the {name} seam", lambda s=seam: s() - 1))
        picks.append((f"behind the {name} seam", lambda s=seam: s()))
    for name, at in picks:
        off = at()
        assert off % PAR_CHUNK in (0, PAR_CHUNK - 1) or off in (0, run.n * REC - 1)
        run.edit(("byte", off, 0x01))
        st = run.fuse(name)
        st.census["byte"] = off


def _capacity(run):
    chunk_seam_map(run, "K>k")
    run.fuse("K>k with cap == n_in, then with room")


BUILDERS = {
    "seam_262144": _seam_262144,
    "chunk_seam": _chunk_seam,
    "shadow_growth": _shadow_growth,
    "fallback_margin": _fallback_margin,
    "guess_series": _guess_series,
    "initialize_map_large": _initialize_map_large,
    "foreign_flags_large": _foreign_flags_large,
    "caller_edits": _caller_edits,
}
CASES = list(BUILDERS)
_BUILT = {}


def build(name):
    """the Steps of a case, built once"""
    if name not in _BUILT:
        run = Run()
        (BUILDERS.get(name) or {"capacity_then_recover": _capacity}[name])(run)
        assert not run.pending
        _BUILT[name] = run.steps
    return _BUILT[name]
