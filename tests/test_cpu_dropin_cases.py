"""The census of tests/dropin_cases.py, asserted on the oracle's results alone: every call of every case enters at the size,
with the holes, the K-against-k relation and the touched fraction it was built for -- so that a device comparison that passes
(tests/test_gpu_dropin_delta.py) has compared what the case claims.  A case that drifts off its thresholds (another scene,
other constants, another frame size) fails here, on the CPU."""
import numpy as np
import pytest

import dropin_cases as dc

ORACLE_BUDGET_S = 60.0


@pytest.fixture(scope="module")
def built(oracle_built):
    return {name: dc.build(name) for name in dc.CASES + ["capacity_then_recover"]}


def _calls(steps):
    return [s for s in steps if s.kind != "resident"]


def _report(name, steps):
    for i, s in enumerate(steps):
        print(f"{name}[{i}] {s.kind} {s.label!r}: n {s.n_in} -> {s.n_out}, K {s.census.get('K')} k {s.census.get('k')}, "
              f"|T| {len(s.T)} of {s.groups_out} groups ({s.ratio:.4f}), built for the {s.expect} path")


@pytest.mark.parametrize("name", dc.CASES + ["capacity_then_recover"])
def test_every_call_is_built_for_its_path(built, name):
    """|T| / groups of the output: below 0.3 wherever the delta path is meant to run (fallback_margin's own two calls apart),
    and T holds whatever a growing call appends"""
    steps = built[name]
    _report(name, steps)
    for i, s in enumerate(_calls(steps)):
        assert 0 <= s.n_in <= dc.CAPACITY - dc.S and s.n_out <= dc.CAPACITY, (name, i)
        if name == "fallback_margin" and i in (0, 2):
            continue
        assert s.expect == "delta" and s.ratio < 0.3, (name, i, s.ratio)
        if s.kind == "fuse_map":
            assert s.n_out == s.n_in + s.census["K"] - s.census["k"]
        if s.n_out > s.n_in:
            assert set(range(s.n_in // 64, s.groups_out)) <= set(s.T.tolist())


def test_seam_262144(built):
    steps = built["seam_262144"]
    L = dc.TAIL_FAST
    assert [s.n_in for s in steps[:3]] == [L - 1, L, L + 1]
    for s in steps[:3]:  # stale records at 0, 63, 64, 262 143, 262 144 (where the map has them) and in the last two groups
        holes = set(s.census["entry_holes"].tolist())
        want = {i for i in (0, 63, 64, L - 1, L) if i < s.n_in}
        assert want <= holes, (s.n_in, want - holes)
        last = (s.n_in - 1) // 64
        assert {h // 64 for h in holes} >= {last, last - 1}
        assert want <= set(s.rec_idx.tolist()), "the records around the seam are in T"
    # the visible block straddles the limit, counted in each call's own input: records in front of the camera up to the
    # entry maps' last records (262 143 and 262 144 themselves were made stale, and those maps end there) ...
    for s in steps[:3]:
        front = s.census["entry_in_front"]
        assert ((front >= L - 40) & (front < L)).sum() >= 35 and front.max() >= L - 3, (s.n_in, front)
    front = steps[5].census["entry_in_front"]  # ... and in the 300 000-record map live ones on both sides of it
    assert steps[5].n_in > L and ((front >= L - 40) & (front < L)).sum() >= 35 and ((front >= L) & (front <= L + 40)).sum() >= 35
    # below -> (at) -> above -> far below -> below -> above -> below, crossing by the frame itself -> above without an edit -> below
    assert [s.n_in > L for s in steps] == [False, False, True, False, False, True, False, True, False]
    cross = steps[6]
    assert cross.n_in <= L < cross.n_out and steps[7].n_in == cross.n_out and not steps[7].edits
    assert steps[3].n_in < steps[2].n_out and steps[4].n_in > steps[3].n_out and steps[5].n_in > steps[4].n_out, "truncation, two appends"


def test_chunk_seam(built):
    steps = built["chunk_seam"]
    C = dc.HOLE_CHUNK
    rel = [np.sign(s.census["K"] - s.census["k"]) for s in steps]
    assert rel == [-1, 1, 1, 0], [(s.census["K"], s.census["k"]) for s in steps]
    for s in steps:
        assert s.n_in > C and s.n_out > C, "two hole chunks on entry and on return"
        by_chunk = s.census["entry_holes_by_chunk"]
        assert len(by_chunk) == 2 and min(by_chunk) >= 1, by_chunk
        front = s.census["entry_in_front"]  # the visible block, live in this call's input on both sides of index 524 288
        assert ((front >= C - 40) & (front < C)).sum() >= 30 and ((front >= C) & (front <= C + 40)).sum() >= 30, (s.label, front)
    for s in (steps[0], steps[1], steps[3]):
        holes = set(s.census["entry_holes"].tolist())
        assert {C - 1, C} <= holes
    assert min(steps[0].census["entry_holes_by_chunk"]) >= 200, "a few hundred holes in each chunk"
    # K < k: the move chain takes records from the end (all of them in chunk 1) into holes of chunk 0
    assert steps[0].census["sources_from"] > C and steps[0].census["moves_into_chunk0"] >= 100, steps[0].census
    # ... and some of the records at the end are holes themselves (a source that is a hole: the chain is followed)
    k_lt = steps[0]
    assert int((k_lt.census["entry_holes"] >= k_lt.n_out).sum()) > k_lt.census["K"]
    # K > k: the old end on a group boundary, then inside a group
    assert steps[1].n_in % 64 == 0 and steps[2].n_in % 64 != 0 and steps[2].n_in == steps[1].n_out
    assert steps[3].n_in == steps[3].n_out and steps[3].census["K"] > 0


def test_shadow_growth(built):
    steps = built["shadow_growth"]
    assert len(steps) == 12
    for j, thr in enumerate((1 << 16, 1 << 17, 1 << 18, 1 << 19)):
        fits, regrows, further = steps[3 * j:3 * j + 3]
        assert fits.n_in + dc.S == thr and regrows.n_in + dc.S == thr + 1
        assert thr < further.n_in + dc.S <= 2 * thr, "the first delta call against the new buffers"
        prev = len(regrows.T)
        assert len(further.T) > prev + prev // 4 + 8 + 100, "more than the guess: a second transfer"
        if j < 3:
            assert len(steps[3 * j + 3].T) * 5 < len(further.T), "then far below the previous count"


def test_fallback_margin(built):
    steps = built["fallback_margin"]
    assert all(s.n_in > dc.TAIL_FAST for s in steps)
    lo, after_lo, hi, after_hi = steps
    assert 0.53 <= lo.ratio <= 0.55 and lo.expect == "delta", lo.ratio
    assert 0.65 <= hi.ratio <= 0.67 and hi.expect == "full", hi.ratio
    assert after_lo.ratio < 0.01 and after_hi.ratio < 0.01 and not after_lo.edits and not after_hi.edits


def test_guess_series(built):
    t = [len(s.T) for s in built["guess_series"]]
    tiny, large, tiny2, zero, large2 = t
    assert 0 < tiny and large > 10 * tiny, t
    assert large > tiny + tiny // 4 + 8, "a second transfer"
    assert 0 < tiny2 and 10 * tiny2 < large, "an oversized first transfer"
    assert zero == 0 and built["guess_series"][3].n_in == built["guess_series"][3].n_out, "nothing to bring back"
    assert large2 > 8 + 100, "a second transfer from guess = 8"
    assert len(built["guess_series"][3].census["entry_holes"]) == 0, "nothing stale or dead under the blind frame"


def test_initialize_map_large(built):
    steps = built["initialize_map_large"]
    assert [s.kind for s in steps] == ["init_map", "fuse_map", "init_map", "fuse_map"]
    first = steps[0]
    assert first.n_in > dc.HOLE_CHUNK and first.n_out == first.n_in, "no compaction"
    assert min(first.census["entry_holes_by_chunk"]) >= 200 and first.census["K"] == len(first.new) > 0
    assert len(first.T) > 300, "the deleted groups come back"
    for init, fuse in (steps[:2], steps[2:]):
        assert fuse.edits and fuse.edits[-1][0] == "size", "the caller's own refill / append loop"
        assert fuse.n_in == init.n_in + init.census["K"] - init.census["k"]


def test_foreign_flags_large(built):
    before, res, after = built["foreign_flags_large"]
    assert res.kind == "resident" and before.n_out > dc.HOLE_CHUNK
    f = res.census["foreign_T"]
    chunk = f * 64 // dc.HOLE_CHUNK
    assert (chunk == 0).sum() >= 200 and (chunk == 1).sum() >= 50, "flags left in both hole chunks"
    assert len(after.T) + 8 < len(f) // 4 and not after.edits, "a call that does not clear them brings far more groups back"


def test_caller_edits(built):
    steps = built["caller_edits"]
    assert len(steps) == 9 and all(s.n_in > dc.TAIL_FAST for s in steps)
    offs = [s.census["byte"] for s in steps[1:]]
    sizes = [s.n_in * dc.REC for s in steps[1:]]
    assert offs[0] == 0 and offs[1] == sizes[1] - 1
    n_seams = [(b - 1) // dc.PAR_CHUNK for b in sizes]
    assert offs[2] == dc.PAR_CHUNK - 1 and offs[3] == dc.PAR_CHUNK
    assert n_seams[4] >= 3 and 1 < n_seams[4] // 2 + 1 < n_seams[4], "a seam strictly between the first and the last"
    assert offs[4] == (n_seams[4] // 2 + 1) * dc.PAR_CHUNK - 1 and offs[5] == (n_seams[5] // 2 + 1) * dc.PAR_CHUNK
    assert offs[6] == n_seams[6] * dc.PAR_CHUNK - 1 and offs[7] == n_seams[7] * dc.PAR_CHUNK and offs[7] < sizes[7]
    assert all(o % dc.REC not in (0, dc.REC - 1) for o in offs[2:]), "a seam falls inside a record"
    for s in steps[1:]:  # without the edit the call would have skipped the upload: one byte is all the caller changed
        assert len(s.edits) == 1 and s.edits[0][0] == "byte"


def test_capacity_case(built):
    (s,) = built["capacity_then_recover"]
    assert s.census["K"] > s.census["k"] and s.n_out > s.n_in > dc.HOLE_CHUNK and min(s.census["entry_holes_by_chunk"]) >= 1


def test_oracle_share(built):
    """the oracle's whole work for the suite (every case built once, probes included)"""
    print(f"oracle time for all cases: {dc.ORACLE_SECONDS[0]:.2f} s")
    assert dc.ORACLE_SECONDS[0] < ORACLE_BUDGET_S


def test_thresholds_are_the_products(built):
    """dropin_cases.py restates the sizes at which the product branches.  They are read back from its sources here, so that a
    constant that moves there fails this test instead of leaving both suites green on cases that compare something else."""
    import os
    import re

    from conftest import ROOT
    csrc = os.path.join(ROOT, "densesurfelmapping_amd", "csrc")
    dev = open(os.path.join(csrc, "dsm_device.h")).read()
    api = open(os.path.join(csrc, "dsm_api.hip")).read()
    m = re.search(r"constexpr int kScanWords = (\d+), kTailChunkWords = (\d+) \* kScanWords, kTailFastWords = (\d+);", dev)
    assert m, "the tail's constants are no longer declared as dropin_cases.py read them"
    scan, chunk_threads, fast = (int(x) for x in m.groups())
    assert fast * 64 == dc.TAIL_FAST and chunk_threads * scan * 64 == dc.HOLE_CHUNK
    m = re.search(r"constexpr size_t kParChunk = 1 << (\d+);", api)
    assert m and 1 << int(m.group(1)) == dc.PAR_CHUNK
    m = re.search(r"size_t cap = h->pin_map_cap \? h->pin_map_cap : \(size_t\)1 << (\d+);\s*while \(cap < map_records\) cap \*= 2;", api)
    assert m and 1 << int(m.group(1)) == dc.SHADOW_FIRST, "the shadow's first size and its doubling"
    assert "int guess = h->dropin_last_groups + h->dropin_last_groups / 4 + 8;" in api, "the first transfer's size"
    assert "(int64_t)n_grp * 64 * 10 > (int64_t)m * 6" in api, "the 60 % rule"
    # the shadow is asked for n_in + S records (dsm_fuse_map_inv), S = the camera's seed count
    assert "size_t n_back = (size_t)n_in + (size_t)S;" in api and dc.S == (dc.CAM.width // 8) * (dc.CAM.height // 8)
