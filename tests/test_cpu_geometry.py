"""The geometry table of tests/geometry_cases.py on the host:

  (a) the census: PortOracle's replay of every geometry's frames meets the conditions under which a comparison at that size
      compares what the size is for (the count of unlabelled border pixels, every seed owns pixels, labels with bit 15 set and
      the top label 65534 where the grid has them, a map that was fused into, stable seeds after the quiet frame);
  (b) where the reference translation unit has been built, it and PortOracle agree at every geometry after every frame --
      labels, seed table, map and new-surfel count, NaN == NaN;
  (c) the bound seed_cell's division by multiplication rests on, for every grid width and seed index dsm_create lets through:
      a proof of the formula, not of the code that uses it."""
import concurrent.futures

import numpy as np
import pytest

import geometry_cases as gc
from conftest import fields_equal

IDS = [g.name for g in gc.GEOMETRIES]


@pytest.fixture(scope="module")
def ob(oracle_built):
    from oracle import bindings
    return bindings


def replay(ob, g, fr, reference=False):
    """[(new count, labels, seeds, map)] after every frame"""
    orc = ob.RefOracle(g.camera) if reference else ob.PortOracle(g.camera)
    lo, out = np.zeros(0, ob.SURFEL_DTYPE), []
    for img, dep, pose, ref in fr:
        lo, k = orc.fuse_map(ref, img, dep, pose, lo)
        out.append((k, orc.labels(), orc.seeds(), lo))
    orc.close()
    return out


def test_table_covers_what_it_names():
    """the table's own arithmetic: every row's grid and seed count are what its line says, the residues and tile remainders the
    issue names occur, and the order is small to large at the expensive end"""
    S = {g.name: (g.gw, g.gh, g.S) for g in gc.GEOMETRIES}
    for name, want in {"24x24": (3, 3, 9), "31x31": (3, 3, 9), "28x29": (3, 3, 9), "29x28": (3, 3, 9), "50x43": (6, 5, 30), "63x27": (7, 3, 21),
                       "64x32": (8, 4, 32), "65x33": (8, 4, 32), "72x56": (9, 7, 63), "64x64": (8, 8, 64), "104x40": (13, 5, 65),
                       "136x120": (17, 15, 255), "128x128": (16, 16, 256), "160x104": (20, 13, 260), "520x24": (65, 3, 195),
                       "24x520": (3, 65, 195), "32767x24": (4095, 3, 12285), "24x32767": (3, 4095, 12285),
                       "2048x1032": (256, 129, 33024), "2040x2056": (255, 257, 65535)}.items():
        assert S[name] == want, name
    assert {s % 4 for _, _, s in S.values()} == {0, 1, 2, 3}  # (every partial last group of k_seed_fit)
    assert {(g.w % 8, g.h % 8) for g in gc.GEOMETRIES} >= {(4, 5), (5, 4), (7, 7), (7, 0), (0, 7)}
    assert any(g.w % 64 == 1 and g.w > 64 for g in gc.GEOMETRIES) and any(g.h % 16 == 1 and g.h % 4 == 1 for g in gc.GEOMETRIES)
    assert gc.unlabelled_pixels(gc.BY_NAME["31x31"]) == 177 and gc.unlabelled_pixels(gc.BY_NAME["28x29"]) == 28
    assert gc.GEOMETRIES[-1].S == gc.MAX_SEEDS and [g.name for g in gc.GEOMETRIES if g.big] == [g.name for g in gc.GEOMETRIES[-4:]]
    for g in gc.GEOMETRIES:
        cam = g.camera
        assert cam.fx != cam.fy and cam.cx != (g.w - 1) / 2 and cam.cy != (g.h - 1) / 2
        assert 0 <= g.quiet_frame < min(4, g.n_frames)


def test_variants_are_distinguishable():
    g = gc.BY_NAME["65x33"]
    runs = [gc.frames(g, 3, v) for v in range(gc.VARIANTS)]
    for a in range(gc.VARIANTS):
        for b in range(a):
            for t in range(3):
                assert not np.array_equal(runs[a][t][0], runs[b][t][0]), (a, b, t)
            assert not np.array_equal(runs[a][1][2], runs[b][1][2])
    again = gc.frames(g, 3, 5)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1], equal_nan=True) for x, y in zip(again, runs[5]))
    dep = runs[0][0][1]
    assert (dep == 0).any() and np.isinf(dep).any() and np.isnan(dep).any()  # holes, unmatched disparities, NaN


@pytest.mark.parametrize("name", IDS)
def test_census_and_reference(ob, name):
    """(a) and (b) on one replay per side: the frame-group run, whose first frames are the run of the other forms"""
    g = gc.BY_NAME[name]
    fr = gc.frames(g, g.group_frames)
    assert (g.n_frames, len(fr)) == ((2, 5) if g.big else (6, 6))
    assert all(np.array_equal(a[1], b[1], equal_nan=True) and np.array_equal(a[2], b[2]) for a, b in zip(gc.frames(g), fr))
    port = replay(ob, g, fr)
    print(name, g.against, "\n   ", gc.census(g, port[:g.n_frames]), "\n   ", gc.census(g, port))
    if not ob.have_ref("serial"):
        return  # (the reference translation unit is built only where its sources are)
    for t, (got, want) in enumerate(zip(port, replay(ob, g, fr, reference=True))):
        assert got[0] == want[0], f"{name} frame {t}: new surfel count {got[0]} vs the reference's {want[0]}"
        assert np.array_equal(got[1], want[1]), f"{name} frame {t}: {int((got[1] != want[1]).sum())} labels differ"
        assert fields_equal(got[2], want[2]) == [], f"{name} frame {t}: seed table differs {fields_equal(got[2], want[2])}"
        assert fields_equal(got[3], want[3]) == [], f"{name} frame {t}: map differs {fields_equal(got[3], want[3])}"


@pytest.mark.parametrize("name", IDS)
def test_census_of_the_other_variants(ob, name):
    """the runs the handles of a batch take beside variant 0: the same conditions.  Among them that no pixel with a candidate
    cell is left without a pick -- a robust mean depth inside (0, 0.05) m puts every cost of a pixel past the reference's 1e6
    sentinel, it indexes seeds[-1] there and the engine refuses the frame (DSM_E_INVALID): such a run would compare nothing."""
    g = gc.BY_NAME[name]
    with concurrent.futures.ThreadPoolExecutor(max_workers=gc.VARIANTS - 1) as ex:  # (ctypes lets go of the GIL)
        for v, c in enumerate(ex.map(lambda v: gc.census(g, replay(ob, g, gc.frames(g, variant=v))), range(1, gc.VARIANTS)), 1):
            print(name, "variant", v, c)


def test_seed_cell_magic_division_bound():
    """seed_cell takes s / gw as mulhi(s, 2^32 // gw + 1).  For every gw from 3 to 21845 (= 65535 // 3) and every seed index s
    below gw * min(65535 // gw, 4095) -- every grid dsm_create accepts: gh >= 3, gh <= 32767 // 8, gw * gh <= 65535 -- the
    product's high word IS the quotient.  Exhaustive, in blocks of grid widths.  (A proof of the formula, not of the code.)"""
    checked = 0
    for lo in range(3, 21846, 64):
        gw = np.arange(lo, min(lo + 64, 21846), dtype=np.uint64)[:, None]
        limit = gw * np.minimum(np.uint64(65535) // gw, np.uint64(4095))
        s = np.arange(int(limit.max()), dtype=np.uint64)[None, :]
        magic = np.uint64(1 << 32) // gw + np.uint64(1)
        assert (magic < np.uint64(1 << 32)).all()  # (it fits the 32-bit operand)
        bad = (((s * magic) >> np.uint64(32)) != s // gw) & (s < limit)
        assert not bad.any(), f"gw {int(gw[np.argwhere(bad)[0][0], 0])}, s {int(np.argwhere(bad)[0][1])}"
        checked += int(limit.sum())
    assert checked > 1_000_000_000
