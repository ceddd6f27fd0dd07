"""The drop-in calls' delta download on large maps and at its branch points (cases: tests/dropin_cases.py, their census:
tests/test_cpu_dropin_cases.py).

dsm_fuse_map keeps three copies of the map equal -- the device map, the page-locked shadow, the caller's array -- and after a
frame brings back only the 64-record groups whose DeviceCtx::grp_dirty flag is set.  A writer that misses a flag leaves the
caller's array and the shadow stale TOGETHER: the next call finds them equal, skips the upload, and host and device differ
from then on without an error anywhere.  So after EVERY call of every case, on one caller-owned buffer of 1 << 20 records:

  * the returned size and new-surfel count are the oracle's;
  * buf[:n] is the oracle's map in every field, byte for byte, NaN == NaN -- and so is the device map itself (map_download);
  * everything behind max(n_in, n_out), rounded up to a group, is what the caller left there (a guard pattern at first);
  * dsm_debug_dropin_stats shows the path the census built the call for: delta or full download; on a delta call at least
    |T| groups came back; where a case is about the first transfer's `guess`, the series of counts holds a delta call with
    more than prev + prev / 4 + 8 groups (the second transfer) and one far below the previous count.

Every case runs eager (flags = 1) and through captured graphs (flags = 0).  The cases cover: the one-workgroup limit of
k_frame_tail from both sides and across map_grows; two hole chunks listed by separate workgroups with K < k (the move chain
from chunk 1 into chunk 0), K == k and K > k; the shadow's regrowth at 65 536, 131 072, 262 144 and 524 288 records; both
sides of the 60 % rule; the guess after a tiny, a large, an empty and a full call; dsm_fuse_initialize_map; flags left by a
resident frame; single-byte caller edits at the seams of the host compare's 1 MiB chunks; DSM_E_CAPACITY and the call after.

Out of scope: maps above 16.7 M surfels, where k_delta_pack's grid-stride loop makes a second trip and k_frame_tail holds
more hole chunks than workgroups -- gigabytes of page-locked memory per handle, not a test of a few seconds.  Batches and
frame groups have no drop-in form.
"""
import ctypes as C

import numpy as np
import pytest

import dropin_cases as dc
from conftest import fields_equal
from test_gpu_parity import mods  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

FORMS = {"eager": 1, "graph": 0}
GUESS_CASES = ("guess_series", "shadow_growth")


def _c_call(api, ff, entry, frame, buf, n, cap):
    """dsm_fuse_map_inv / dsm_fuse_initialize_map_inv on the caller's own array, status code handed back: (rc, n, new surfels)"""
    t, img, dep, pose, ref = frame
    img, dep = ff._frame_args(img, dep)
    pose_cm = api.pose_to_colmajor(pose)
    n_new = C.c_int32(0)
    head = (ff._h, ref, api._ptr(img), img.strides[0], api._ptr(dep), dep.strides[0], api._ptr(pose_cm), None, api._ptr(buf))
    if entry == "fuse_map":
        n_io = C.c_int32(n)
        rc = ff._lib.dsm_fuse_map_inv(*head, C.byref(n_io), cap, C.byref(n_new))
        return rc, n_io.value, n_new.value
    fresh = np.zeros(ff.n_seed, api.SURFEL_DTYPE)
    rc = ff._lib.dsm_fuse_initialize_map_inv(*head, n, api._ptr(fresh), len(fresh), C.byref(n_new))
    return rc, n, fresh[:n_new.value]


def _guard_intact(buf, model, n_in, n_out):
    hi = -(-max(n_in, n_out) // dc.GROUP) * dc.GROUP
    return np.array_equal(dc.raw(buf[hi:]), dc.raw(model[hi:]))


def _run(mods, name, form):
    api, synth, ob = mods
    steps = dc.build(name)
    ff = api.FusionFunctions.from_camera(dc.CAM, flags=FORMS[form], frame_slots=2, surfel_capacity=dc.CAPACITY)
    buf, model = dc.guard_buffer(api.SURFEL_DTYPE), dc.guard_buffer(api.SURFEL_DTYPE)  # the caller's array; what it must hold
    n, series = 0, []
    try:
        for i, s in enumerate(steps):
            tag = f"{name} {form} call {i} ({s.label})"
            t, img, dep, pose, ref = s.frame
            if s.kind == "resident":  # behind the shadow's back: a foreign map, a resident frame on it, the caller's state again
                foreign = buf[:n].copy()
                dc.apply_edits(foreign, n, s.foreign_edits)
                ff.map_upload(foreign)
                ff.frame_upload(0, img, dep)
                ff.fuse_frame_resident(0, ref, pose)
                ff.synchronize()
                ff.map_upload(buf[:n])
                continue
            n = dc.apply_edits(buf, n, s.edits)
            dc.apply_edits(model, 0, s.edits)
            assert n == s.n_in, tag
            before = ff.debug_dropin_stats()
            if s.kind == "fuse_map":
                n_out, k = ff.fuse_map_inplace(ref, img, dep, pose, buf, n)
            else:
                rc, n_out, new = _c_call(api, ff, "init_map", s.frame, buf, n, n)
                ff._check(rc)
                k = len(new)
            after = ff.debug_dropin_stats()
            model[s.rec_idx] = s.recs.astype(api.SURFEL_DTYPE)
            took_delta = after["delta_calls"] - before["delta_calls"]
            last = after["last_groups"]
            print(f"{tag}: n {s.n_in} -> {n_out}, |T| {len(s.T)}, last_groups {last}, previous {before['last_groups']}, "
                  f"{'delta' if took_delta else 'full'} download")
            assert (n_out, k) == (s.n_out, s.k_new), f"{tag}: size / new surfels {(n_out, k)}, the oracle's {(s.n_out, s.k_new)}"
            if took_delta:
                assert last >= len(s.T), f"{tag}: {last} groups came back, the oracle changed {len(s.T)}"
            bad = fields_equal(buf[:n_out], model[:n_out])
            assert bad == [], f"{tag}: the caller's array differs from the oracle's map {bad}"
            if s.kind == "init_map":
                assert fields_equal(new, s.new.astype(api.SURFEL_DTYPE)) == [], f"{tag}: new surfels"
            assert _guard_intact(buf, model, s.n_in, n_out), f"{tag}: written behind the map's end"
            bad = fields_equal(ff.map_download(), model[:n_out])
            assert bad == [], f"{tag}: the DEVICE map differs from the oracle's {bad}"
            assert after["calls"] == before["calls"] + 1, tag
            assert took_delta == (1 if s.expect == "delta" else 0), \
                f"{tag}: built for the {s.expect} download, |T| {len(s.T)} of {s.groups_out} groups, the device counted {last}"
            if name == "foreign_flags_large" and i == len(steps) - 1:
                # every flag of this call is a changed record's (in T), or a refill / append target in the last group: the
                # resident frame's hundreds of flags were cleared before the frame ran
                assert last <= len(s.T) + 8, f"{tag}: {last} groups back, {len(s.T)} changed"
            series.append((before["last_groups"], last, took_delta))
            n = n_out
        if name in GUESS_CASES:
            assert any(d and cur > prev + prev // 4 + 8 for prev, cur, d in series), ("no call needed a second transfer", series)
            assert any(cur * 5 < prev for prev, cur, d in series), ("no call came in far below its first transfer", series)
    finally:
        ff.close()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", dc.CASES)
def test_dropin_delta(mods, name, form):  # noqa: F811
    _run(mods, name, form)


def test_capacity_then_recover(mods):  # noqa: F811
    """A K > k call on the chunk_seam map through the C entry point with cap == n_in: DSM_E_CAPACITY, *n_local = the size
    needed, the caller's whole buffer untouched.  The same call again with room, on the array as the failed call left it, gives
    the oracle's result for the caller's unchanged input: the device map had moved on, the shadow must not be trusted."""
    api, synth, ob = mods
    (s,) = dc.build("capacity_then_recover")
    ff = api.FusionFunctions.from_camera(dc.CAM, frame_slots=2, surfel_capacity=dc.CAPACITY)
    buf, model = dc.guard_buffer(api.SURFEL_DTYPE), dc.guard_buffer(api.SURFEL_DTYPE)
    try:
        n = dc.apply_edits(buf, 0, s.edits)
        dc.apply_edits(model, 0, s.edits)
        assert n == s.n_in and s.n_out > n
        rc, needed, _ = _c_call(api, ff, "fuse_map", s.frame, buf, n, n)
        assert rc == api.DSM_E_CAPACITY, rc
        assert needed == s.n_out, f"needed size reported as {needed}, the oracle's map has {s.n_out}"
        # include/dsm.h: local[] is left as it was handed in (stricter than "except for groups the oracle also changes") -- and
        # the second call runs on the array the failed one left
        assert np.array_equal(dc.raw(buf), dc.raw(model)), "the failed call wrote to the caller's array"
        before = ff.debug_dropin_stats()
        rc, n_out, k = _c_call(api, ff, "fuse_map", s.frame, buf, n, len(buf))
        ff._check(rc)
        after = ff.debug_dropin_stats()
        model[s.rec_idx] = s.recs.astype(api.SURFEL_DTYPE)
        print(f"capacity_then_recover: n {n} -> {n_out}, |T| {len(s.T)}, last_groups {after['last_groups']}, previous {before['last_groups']}")
        assert (n_out, k) == (s.n_out, s.k_new)
        assert fields_equal(buf[:n_out], model[:n_out]) == [], fields_equal(buf[:n_out], model[:n_out])
        assert _guard_intact(buf, model, n, n_out)
        assert fields_equal(ff.map_download(), model[:n_out]) == []
        assert after["delta_calls"] == before["delta_calls"] + 1 and after["last_groups"] >= len(s.T)
    finally:
        ff.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_handle_capacity_leaves_the_callers_count(mods, form):  # noqa: F811
    """The other source of DSM_E_CAPACITY: the HANDLE's surfel_capacity (8 192 here), not the caller's array, cannot hold
    n_in + K - k.  No count is known then: *n_local and *n_new stay as they were handed in (a caller that took *n_local for
    the size needed would hand an empty map back), the caller's array is untouched, and the error is reported once: the next
    call, on a map cut so that it fits, gives the oracle's result."""
    api, synth, ob = mods
    hcap = 8192
    ff = api.FusionFunctions.from_camera(dc.CAM, flags=FORMS[form], frame_slots=2, surfel_capacity=hcap)
    try:
        assert ff.map_capacity() == hcap
        buf = np.full((hcap + dc.S) * dc.REC, dc.GUARD_BYTE, np.uint8).view(api.SURFEL_DTYPE)
        n = hcap - 5
        buf[:n] = dc._parked(ob, n, 5)
        keep = buf.copy()
        frame = dc.frames()[3]
        t, img, dep, pose, ref = frame
        lo, k_new = ob.PortOracle(dc.CAM).fuse_map(ref, img, dep, pose, keep[:n].astype(ob.SURFEL_DTYPE))
        assert len(lo) > hcap and len(lo) <= len(buf), "the frame was to outgrow the handle, not the caller's array"
        rc, n_after, _ = _c_call(api, ff, "fuse_map", frame, buf, n, len(buf))
        assert rc == api.DSM_E_CAPACITY, rc
        assert n_after == n, f"*n_local became {n_after}: no size is known when the handle's capacity is the limit"
        assert np.array_equal(dc.raw(buf), dc.raw(keep)), "the failed call wrote to the caller's array"
        n = hcap - 100
        lo, k_new = ob.PortOracle(dc.CAM).fuse_map(ref, img, dep, pose, keep[:n].astype(ob.SURFEL_DTYPE))
        assert len(lo) < hcap
        rc, n_out, k = _c_call(api, ff, "fuse_map", frame, buf, n, len(buf))
        ff._check(rc)
        assert (n_out, k) == (len(lo), k_new)
        assert fields_equal(buf[:n_out], lo.astype(api.SURFEL_DTYPE)) == []
        assert fields_equal(ff.map_download(), lo.astype(api.SURFEL_DTYPE)) == []
        hi = -(-max(n, n_out) // dc.GROUP) * dc.GROUP
        assert np.array_equal(dc.raw(buf[hi:]), dc.raw(keep[hi:]))
    finally:
        ff.close()
