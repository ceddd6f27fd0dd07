"""Generate tests/golden/ref_tu_traces.json from the REFERENCE's own translation unit.

Runs only where /root/reference exists: oracle/_ref/libdsm_ref_serial*.so is surfel_fusion/src/fusion_functions.cpp compiled
in place (oracle/Makefile, `make ref`).  The traces are digests of what that TU computes on the sequences and states of
tests/test_cpu.py::test_port_oracle_matches_reference_tu and ::test_reference_quirk_states, so that those tests compare the
C restatement with the reference wherever the reference itself is absent.

    python tests/golden/make_golden_ref_tu.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "ref_tu_traces.json")
# (camera, scene seed, frames): TINY_RAGGED has (size mod 8) > 4, where the reference touches superpixel_seeds[-1]
SEQUENCES = [("TINY", 3, 40), ("KITTI_1241", 4, 3), ("TINY_RAGGED", 3, 12)]
QUIRK_TRIALS = 6


def digest(a: np.ndarray) -> str:
    """SHA-256 of an array, field by field, with every NaN replaced by one canonical NaN (the reference's arithmetic does not
    define a NaN's sign or payload): two arrays have the same digest exactly when conftest.fields_equal finds no difference"""
    h = hashlib.sha256()
    names = a.dtype.names or (None,)
    for f in names:
        x = np.ascontiguousarray(a if f is None else a[f])
        if x.dtype.kind == "f":
            x = x.copy()
            bits = x.view(np.uint32 if x.itemsize == 4 else np.uint64)
            bits[np.isnan(x)] = 0x7FC00000 if x.itemsize == 4 else 0x7FF8000000000000
            x = bits
        h.update(x.tobytes())
    return h.hexdigest()


def sequence_trace(orc, cam, scene, n, synth, surfel_dtype):
    """per frame: [new surfels, map size, labels, seeds, map] of an oracle replaying the sequence"""
    local, rows = np.zeros(0, surfel_dtype), []
    for t, img, dep, pose, ridx in synth.sequence(cam, scene, n):
        local, k = orc.fuse_map(ridx, img, dep, pose, local)
        rows.append([int(k), int(len(local)), digest(orc.labels()), digest(orc.seeds()), digest(local)])
    return rows


def quirk_trace(make_oracle, cam, synth):
    """The two scheduling quirks: random stable flags + random labels, and an unstable seed that owns no
    pixel mid-chunk, each trial on a fresh oracle from make_oracle(cam); per trial the digests of the state after each step.
    The random draws depend on the number of seeds only, so every oracle is driven through the same states."""
    img, dep, _ = synth.render(cam, synth.Scene(seed=8), 0)
    rng = np.random.default_rng(0)
    rows = []
    for trial in range(QUIRK_TRIALS):
        orc = make_oracle(cam)
        orc.set_frame(img, dep)
        orc.stage("initialize_seeds")
        orc.stage("update_pixels")
        orc.stage("update_seeds")
        seeds, labels = orc.seeds(), orc.labels()
        row = [digest(seeds), digest(labels)]
        seeds["stable"] = rng.random(len(seeds)) < 0.5
        victim = int(rng.integers(0, len(seeds)))
        seeds["stable"][victim] = 0
        gw = cam.width // 8
        neighbour = victim + 1 if (victim % gw) + 1 < gw else victim - 1
        labels[labels == victim] = neighbour  # victim now owns nothing
        orc.set_seeds(seeds)
        orc.set_labels(labels)
        orc.stage("update_seeds")
        row.append(digest(orc.seeds()))
        orc.stage("update_pixels")
        row += [digest(orc.labels()), digest(orc.seeds())]
        rows.append(row)
    return rows


def main():
    from densesurfelmapping_amd import synth
    from oracle.bindings import SURFEL_DTYPE, RefOracle
    out = {"generator": "oracle/_ref/libdsm_ref_serial*.so (reference fusion_functions.cpp, serial thread schedule)",
           "sequences": [{"camera": c, "scene_seed": s, "frames": n,
                          "trace": sequence_trace(RefOracle(getattr(synth, c)), getattr(synth, c), synth.Scene(seed=s), n, synth, SURFEL_DTYPE)}
                         for c, s, n in SEQUENCES],
           "quirk_states": {"camera": "TINY", "trace": quirk_trace(RefOracle, synth.TINY, synth)}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
