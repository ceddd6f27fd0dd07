"""The inputs of tests/test_gpu_sequence_walk.py without a GPU (tests/sequence_cases.py): every member of every sequence shows in
the index plane of the render's and of the grid's host checker on its own, so that plane pins every sequence number; and the
cases are the ones the walk of csrc/dsm_k_sequence.h turns on."""
import numpy as np
import pytest

import sequence_cases as sc

CASES = sc.cases()


@pytest.fixture(scope="module")
def dtype():
    from densesurfelmapping_amd import api
    assert api.CLOUD_TILE == sc.T
    return api.SURFEL_DTYPE


@pytest.mark.parametrize("product", ["render", "grid"])
def test_every_member_shows_on_its_own(dtype, product):
    place = sc.PLACE[product]
    store = sc.store_records(dtype, place)
    for name, ut, segs in CASES:
        m = place(dtype, ut)
        seq = sc.sequence(store, m, segs)
        assert len(seq) == sc.run_total(segs) + int((ut >= 5).sum()), name
        exp = sc.expected(product, seq)  # asserts: as many distinct indices as members
        # and the numbers are the sequence's: member k sits where its record was placed
        k = np.arange(len(seq))
        slot = np.concatenate([sc.SLOTS - 1 - np.arange(b, b + c) for b, c in segs] + [np.nonzero(ut >= 5)[0]]).astype(np.int64)
        assert np.array_equal(exp["index"].ravel()[slot], k), name
        assert (np.delete(exp["index"].ravel(), slot) == -1).all(), name


def test_cases_are_the_walks_edges():
    T = sc.T
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)
    assert [len(ut) for _, ut, segs in CASES if not segs][:12] == [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]
    assert {sc.run_total(segs) for segs in sc.RUNS.values()} == {0, 1, 63, 64, 65}
    for segs in list(sc.RUNS.values()) + [sc.FRONT]:
        named = np.concatenate([np.arange(b, b + c) for b, c in segs] + [np.zeros(0, int)])
        assert len(np.unique(named)) == len(named) and (named < sc.STORE_N).all(), segs  # no store record twice
    assert any(len(segs) > 1 and all(c == 1 for _, c in segs) for segs in sc.RUNS.values())
    assert any(any(c == 0 for _, c in segs) and any(c > 0 for _, c in segs) for segs in sc.RUNS.values())
    assert any(len(segs) == 2 and 0 < segs[0][1] < 64 for segs in sc.RUNS.values())  # a boundary inside a wave's 64 outputs
    p = {k: v >= 5 for k, v in sc.PATTERNS.items()}
    assert all(len(v) == 5 * T + 3 for v in p.values())
    assert not p["none pass"].any() and p["all pass"].all()
    assert p["alternating"][::2].all() and not p["alternating"][1::2].any()
    assert np.array_equal(np.nonzero(p["every 64th"])[0] % 64, np.full(len(p["every 64th"]) // 64, 63))
    # the 256 records of one wave (four chunks of 64 of one tile quarter), a whole tile: failing between passing ones
    assert np.array_equal(np.nonzero(~p["one wave failing"])[0], np.arange(T + 256, T + 512))
    assert np.array_equal(np.nonzero(~p["one tile failing"])[0], np.arange(2 * T, 3 * T))
