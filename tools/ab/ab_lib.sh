#!/bin/bash
# interleaved A/B of two library builds on one box: headline bench, Merkle / LDE kernel ms and total
O=${1:-${TMPDIR:-/tmp}/nx_ab}; mkdir -p "$O"   # where the bench lines land
for round in 1 2 3; do
  for lib in old new; do
    if [ $lib = old ]; then export NX_LIB=$PWD/nexus-zkvm_amd/libnexus_hip_old.so; else unset NX_LIB; fi
    timeout 300 python bench.py --full --no-cpu-baseline --no-v1-shaped --steps 10 2>&1 | tail -1 > $O/$lib$round.json
    python - <<PY
import json
d=json.load(open("$O/$lib$round.json"))
print("$lib", $round, "ms", round(d["ms_per_step"],3), "merkle", round(d["merkle"]["kernel_ms"],3), "lde", round(d["roofline"]["kernel_ms"],3), d["stages_ms"]["commit"])
PY
  done
done
