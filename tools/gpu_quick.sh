#!/bin/bash
# usage (GPU box, repo root): tools/gpu_quick.sh <tag> [pytest -k expr]
# quick iteration loop: a parity subset, then a short bench with per-kernel event times; logs go to $OUT_DIR (default out/)
tag=$1; kexpr=${2:-"tiny_sequence or resident_replay_kitti or state_level or quiet_scene or golden_fixture"}
out=${OUT_DIR:-out}
mkdir -p "$out"
timeout 600 python -m pytest tests/test_gpu_parity.py -m gpu -x -q -k "$kexpr" 2>&1 | tail -6 > "$out/quick_$tag.test"
cat "$out/quick_$tag.test"
timeout 300 python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-dropin > "$out/quick_$tag.json" 2> "$out/quick_$tag.err"
python - "$out/quick_$tag.json" <<PY
import json, sys
d=json.load(open(sys.argv[1]))
print("fps", d["value"], "sum_us", d["frame_kernel_sum_us"])
print({k: v for k, v in d["kernel_us"].items()})
PY
