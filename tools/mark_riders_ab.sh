cd "$(dirname "$0")/.."
OUT=${OUT_DIR:-bench_out}/r06m; mkdir -p $OUT
for rep in 1 2; do for mr in 256 0 512 1024; do
  E=""; [ $mr != 0 ] && E="NVBX_MARK_RIDERS=$mr"
  env $E timeout 300 python bench.py --scene hall --full --no-cpu-baseline --no-parity > $OUT/hall_$mr.json 2>/dev/null
  env $E timeout 300 python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-parity > $OUT/k20_$mr.json 2>/dev/null
  python - <<PY
import json
h=json.load(open("$OUT/hall_$mr.json")); r=json.load(open("$OUT/k20_$mr.json"))
print("riders $mr (0 = adaptive): hall", h.get("ms_per_step_blocks", h["ms_per_step"]), round(h["kernels"]["k_mark_view"]["avg_us"],1), "| room k20", r.get("ms_per_step_blocks", r["ms_per_step"]), round(r["kernels"]["k_mark_view"]["avg_us"],1))
PY
done; done
