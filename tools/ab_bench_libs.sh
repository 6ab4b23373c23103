set -u
R="$(cd "$(dirname "$0")/.." && pwd)"; cd "$R"; OUT=${1:?usage: tools/ab_bench_libs.sh OUT_DIR}; mkdir -p "$OUT"
for r in 1 2; do for name in ${WAX_AB_LIBS:-base lanes}; do
WAX_HIP_LIB=$R/wax_amd/lib/exp/libwaxhip_$name.so timeout 600 python bench.py --full --gpus 1 --rows 1000000 --steps 60 --warmup 10 --no-cpu-baseline --traffic off --secondary ${WAX_AB_SEC:-b1m_q256,b1m_q1024,c5_shard,clustered_k100,dups17} --detail-out "$OUT/d_${name}_$r.json" > "$OUT/l_${name}_$r.json" 2> /dev/null
python - <<PY
import json
d=json.load(open("$OUT/l_${name}_$r.json"))
print("$name", $r, [(s["name"], s["ms_per_step"], s["kernel_avg_ms"], s.get("blocking_ms"), s["ck"]) for s in d["secondary"]])
PY
done; done
