"""Generate tests/golden/eigen33_* from the REFERENCE's own translation units built against an Eigen >= 3.3 stand-in.

Eigen 3.3 / 3.4 evaluate a small fixed 3x3 * 3x1 product coefficient by coefficient as a redux of length 3, which they split
at 1: a0*b0 + (a1*b1 + a2*b2).  oracle/shims/Eigen restates Eigen 3.2's left-to-right (a0*b0 + a1*b1) + a2*b2.
tests/eigen33/Eigen is that shim with only the two 3x3 * 3x1 operator* bodies changed.  This script compiles
oracle/ref_driver.cpp and oracle/ref_map_driver.cpp + ref_map_ff.cpp with oracle/Makefile's REF_FLAGS twice, into a
temporary directory: once with tests/eigen33 in front of oracle/shims and once without (the default-shim twin).  It runs
both on the cases of tests/eigen33_cases.py, records the Eigen >= 3.3 results, reports how many surfels the product order
moves, and fails if a fixture equals its twin (such a fixture would show nothing).

Runs only where the reference sources exist; the fixtures travel to the GPU box, the reference does not.

    python tests/golden/make_golden_eigen33.py
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from densesurfelmapping_amd import api, synth  # noqa: E402
from oracle import bindings  # noqa: E402
import eigen33_cases as E  # noqa: E402
import node_state  # noqa: E402

ORACLE = os.path.join(ROOT, "oracle")
STANDIN = os.path.join(ROOT, "tests", "eigen33")


def ref_flags():
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", ORACLE, "--eval", "print-ref-flags: ; @echo $(REF_FLAGS)", "print-ref-flags"],
                         check=True, capture_output=True, text=True).stdout
    return out.split()


def build(td, variant):
    """the four reference libraries this script drives; variant "e33" puts tests/eigen33 in front of oracle/shims"""
    flags = ref_flags()
    shims = "-I" + os.path.join(ORACLE, "shims")
    assert flags.count(shims) == 1, flags
    if variant == "e33":
        flags.insert(flags.index(shims), "-I" + STANDIN)
    cxx = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
    libs = {}
    for kind, defs, srcs in [("serial", ["-DDSM_ORACLE_SERIAL_THREADS"], ["ref_driver.cpp"]),
                             ("serial_rgbd", ["-DDSM_ORACLE_SERIAL_THREADS", "-DDSM_REF_RGBD"], ["ref_driver.cpp"]),
                             ("map", ["-DDSM_ORACLE_DEFERRED_THREADS"], ["ref_map_driver.cpp", "ref_map_ff.cpp"])]:
        out = os.path.join(td, f"libdsm_ref_{kind}_{variant}.so")
        subprocess.run([cxx] + flags + defs + ["-o", out] + [os.path.join(ORACLE, s) for s in srcs], check=True)
        libs[kind] = out
    return libs


class Ref(bindings._Base):
    prefix = "dsmref_"

    def __init__(self, cam, libs):
        super().__init__(C.CDLL(libs["serial_rgbd" if cam.rgbd else "serial"]), cam)


def run_sequence(case, libs):
    cam = getattr(synth, case["camera"])
    ref = Ref(cam, libs)
    local = np.zeros(0, bindings.SURFEL_DTYPE)
    per_frame = []
    for t, img, dep, pose, ridx in E.sequence(case, synth):
        local, k = ref.fuse_map(ridx, img, dep, pose, local)
        per_frame.append(E.frame_record(k, local.astype(api.SURFEL_DTYPE), ref.labels(), ref.seeds().astype(api.SEED_DTYPE)))
    ref.close()
    return per_frame, local.astype(api.SURFEL_DTYPE)


def run_edges(camera, libs):
    """{case: (two frame records, final map)}; edge_cases comes from the GPU parity tests (the same frames they feed)"""
    from test_gpu_parity import edge_cases
    cam = getattr(synth, camera)
    out = {}
    for name, (img, dep) in edge_cases(cam).items():
        ref = Ref(cam, libs)
        local = np.zeros(0, bindings.SURFEL_DTYPE)
        steps = []
        for ridx in (0, 1):
            local, k = ref.fuse_map(ridx, img, dep, E.EDGE_POSES[ridx], local)
            steps.append(E.frame_record(k, local.astype(api.SURFEL_DTYPE), ref.labels(), ref.seeds().astype(api.SEED_DTYPE)))
        ref.close()
        out[name] = (steps, local.astype(api.SURFEL_DTYPE))
    return out


def run_node(libs):
    case = next(c for c in node_state.SCENARIOS if c["name"] == E.NODE_SCENARIO)
    assert "camera" not in case  # NODE_CAM: the non-RGB-D node library
    return E.run_node(lambda cam, d: bindings.RefSurfelMap(cam, drift_free_poses=d, lib_path=libs["map"]), synth, node_state)


def main():
    out = {"generator": "reference fusion_functions.cpp / surfel_map.cpp (oracle/ref_driver.cpp, ref_map_driver.cpp + ref_map_ff.cpp, "
                        "serial / deferred thread schedule) built with oracle/Makefile's REF_FLAGS and tests/eigen33 in front of oracle/shims",
           "sequences": [], "edge_cases": [], "node": None}
    same = []
    with tempfile.TemporaryDirectory() as td:
        e33, dflt = build(td, "e33"), build(td, "default")
        for case in E.SEQUENCES:
            pf, final = run_sequence(case, e33)
            pf0, final0 = run_sequence(case, dflt)
            fname = None
            if final.nbytes <= E.MAX_STORED_MAP_BYTES:
                fname = "eigen33_" + case["name"] + "_final_map.npy"
                np.save(os.path.join(HERE, fname), final)
            rec = dict(case, per_frame=pf, final_map=fname, final_n=len(final), final_sha256=E.fields_digest(final),
                       surfels_changed=E.rows_differing(final, final0),
                       frames_changed=sum(a != b for a, b in zip(pf, pf0)))
            out["sequences"].append(rec)
            if pf == pf0:
                same.append(case["name"])
            print(f"{case['name']}: {len(final)} surfels, {rec['surfels_changed']} differ from the default shim's map, "
                  f"{rec['frames_changed']} of {len(pf)} frame records differ")
        for camera in E.EDGE_CAMERAS:
            got, got0 = run_edges(camera, e33), run_edges(camera, dflt)
            fname = "eigen33_edges_" + camera.lower() + ".npz"
            np.savez_compressed(os.path.join(HERE, fname), **{k: v[1] for k, v in got.items()})
            cases = {k: {"steps": v[0], "surfels_changed": E.rows_differing(v[1], got0[k][1])} for k, v in got.items()}
            rec = {"camera": camera, "final_maps": fname, "cases": cases,
                   "surfels_changed": sum(c["surfels_changed"] for c in cases.values())}
            out["edge_cases"].append(rec)
            if all(v[0] == got0[k][0] for k, v in got.items()):
                same.append("edges " + camera)
            print(f"edge cases at {camera}: " + ", ".join(f"{k} {c['surfels_changed']}" for k, c in cases.items()))
        briefs, checkpoints, final, files = run_node(e33)
        briefs0, _, final0, files0 = run_node(dflt)
        fname = "eigen33_node_" + E.NODE_SCENARIO + "_final.npz"
        np.savez_compressed(os.path.join(HERE, fname), **final)
        changed = {}
        for k in final:
            a, b = final[k], final0[k]
            if a.dtype.names:
                changed[k] = E.rows_differing(a, b)
            elif a.shape != b.shape:
                changed[k] = "shape %s vs %s" % (a.shape, b.shape)
            else:
                same_el = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
                changed[k] = int((~same_el).sum())
        out["node"] = {"name": E.NODE_SCENARIO, "briefs": briefs, "checkpoints": checkpoints, "final": fname,
                       "final_digest": node_state.digest(final), "files": files, "records_changed": changed,
                       "files_changed": {k: files[k]["sha256"] != files0[k]["sha256"] for k in files}}
        if node_state.digest(final) == node_state.digest(final0):
            same.append("node " + E.NODE_SCENARIO)
        print(f"node {E.NODE_SCENARIO}: {briefs[-1]}; records that differ from the default shim's node: {changed}; "
              f"files differ: {out['node']['files_changed']}")
    with open(os.path.join(HERE, "eigen33_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
    if same:
        raise SystemExit(f"fixtures equal to their default-shim twins (they would show nothing): {same}")


if __name__ == "__main__":
    main()
