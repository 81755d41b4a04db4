#!/bin/bash
# A/B of two library builds on the room, the hall and the 8-camera batch in ONE box session.   usage: tools/books_ab.sh TAG v0 v1
cd "$(dirname "$0")/.."
TAG=$1; shift; OUT=${OUT_DIR:-bench_out}/$TAG; mkdir -p $OUT
for rep in 1 2; do for v in "$@"; do
  L=$PWD/isaac_ros_nvblox_amd/variants/libnvblox_hip_$v.so; [ $v = current ] && L=$PWD/isaac_ros_nvblox_amd/libnvblox_hip.so
  NVBX_LIB=$L timeout 300 python bench.py --full --no-cpu-baseline --no-parity > $OUT/room_$v.json 2>/dev/null
  NVBX_LIB=$L timeout 300 python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-parity > $OUT/k20_$v.json 2>/dev/null
  NVBX_LIB=$L timeout 300 python bench.py --scene hall --full --no-cpu-baseline --no-parity > $OUT/hall_$v.json 2>/dev/null
  NVBX_LIB=$L timeout 300 python bench.py --workload multicam --cameras 8 --steps 100 --warmup 20 --no-cpu-baseline --no-parity > $OUT/m8_$v.json 2>/dev/null
  python - <<PY
import json
o = []
for w in ("room", "k20", "hall", "m8"):
    d = json.load(open("$OUT/%s_$v.json" % w)); o.append("%s %.4f (fused %.1f us)" % (w, d.get("ms_per_step_blocks", d["ms_per_step"]), d["kernels"]["k_integrate_tsdf_color"]["avg_us"]))
print("$v:", " | ".join(o))
PY
done; done
