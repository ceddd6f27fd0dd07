"""The label image of a sweep >= 1 without a pass over every pixel: a numpy model of what k_assign and k_resolve do
(dsm_k_superpixel.h, resolve_worklist) against the reference's sequential scan (FF.cpp:400,445,450), the formula of
test_cpu.py::test_stable_skip_fixed_point_bruteforce.

k_assign settles the pixels in no particular order.  A pixel whose old seed was unstable at sweep start stores its pick
as its label on the spot; a pixel whose old seed was stable and which picks another seed goes onto the list with its pick
in the sparse `cand` plane; k_resolve iterates the list to the fixed point of tmin and then stores the picks that count."""
import numpy as np

INF = 2 ** 31 - 1
UNSET = -7  # what the sparse pick plane holds where nothing was stored: must never reach a label


def _reference_scan(old, pick, stable0):
    """Row-major scan: labels, stable flags afterwards, and T[s] = the pixel at which s lost `stable` (-1 / INF)."""
    st = stable0.copy()
    lab = old.copy()
    t_final = np.where(stable0, INF, -1).astype(np.int64)
    for p in range(len(old)):
        if st[lab[p]]:
            continue
        lab[p] = pick[p]
        if st[pick[p]]:
            st[pick[p]] = False
            t_final[pick[p]] = p
    return lab, st, t_final


def _device_model(rng, old, pick, stable0, t_final):
    n_pix = len(old)
    tmin = np.where(stable0, INF, -1).astype(np.int64)
    label = old.copy()  # updated in place
    cand = np.full(n_pix, UNSET, np.int64)
    work = []
    # ---- k_assign: every pixel once, any order
    for p in rng.permutation(n_pix):
        l, c = label[p], pick[p]  # (a pixel's label is read at the pixel itself only: still the old one)
        assert l == old[p]
        # tmin[l] as this thread happens to see it: -1 for the whole sweep, or anything between +inf and where it ends up
        tl = -1 if not stable0[l] else int(rng.integers(t_final[l], INF, endpoint=True))
        if tl == -1:
            if c != l:
                label[p] = c
            if tmin[c] > p:
                tmin[c] = p
        elif c != l:
            cand[p] = c
            work.append(int(p))
    # ---- k_resolve: the fixed point over the list (entries in any order) ...
    changed = True
    while changed:
        changed = False
        for i in rng.permutation(len(work)):
            p = work[i]
            if tmin[label[p]] < p and tmin[cand[p]] > p:
                tmin[cand[p]] = p
                changed = True
    # ... and the listed pixels' labels
    for i in rng.permutation(len(work)):
        p = work[i]
        if tmin[label[p]] < p:
            label[p] = cand[p]
    return label, tmin, work


def test_in_place_labels_match_the_sequential_scan():
    rng = np.random.default_rng(11)
    listed = stable_changed = 0
    for trial in range(400):
        n_seed = int(rng.integers(2, 12))
        n_pix = int(rng.integers(1, 200))
        old = rng.integers(0, n_seed, n_pix)
        pick = rng.integers(0, n_seed, n_pix)
        stable0 = rng.random(n_seed) < rng.uniform(0.0, 1.0)
        if trial % 50 == 0:
            stable0[:] = False
        if trial % 50 == 1:
            stable0[:] = True
        lab_ref, st, t_final = _reference_scan(old, pick, stable0)
        label, tmin, work = _device_model(rng, old, pick, stable0, t_final)
        assert np.array_equal(label, lab_ref), trial
        assert np.array_equal(tmin == INF, st), trial
        assert np.array_equal(tmin, t_final), trial
        assert (label != UNSET).all(), trial
        # the list: no pixel whose old seed was unstable, no pixel twice, every pixel that could still change
        assert all(stable0[old[p]] for p in work), trial
        assert len(set(work)) == len(work), trial
        assert set(work) == set(np.nonzero(stable0[old] & (pick != old))[0].tolist()), trial
        listed += len(work)
        stable_changed += int((stable0[old] & (label != old)).sum())
        if stable0.all():
            assert np.array_equal(label, old), trial
        if not stable0.any():
            assert not work and np.array_equal(label, pick), trial
    # (not vacuous: the fixed point decided labels both ways)
    assert stable_changed > 1000 and listed - stable_changed > 1000, (listed, stable_changed)
