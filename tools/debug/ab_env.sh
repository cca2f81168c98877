# A/B an environment setting on one box: tools/debug/ab_env.sh VAR=value [bench args...]
# Writes ab_{base,alt}_<rep>.json and ab.err into $OUT (default bench_out/).
set -e
KV=$1; shift
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for rep in 1 2; do
  python bench.py --full --no-cpu-baseline --steps 64 --warmup 8 --no-prefill-timing "$@" > "$OUT/ab_base_$rep.json" 2>> "$OUT/ab.err"
  env $KV python bench.py --full --no-cpu-baseline --steps 64 --warmup 8 --no-prefill-timing "$@" > "$OUT/ab_alt_$rep.json" 2>> "$OUT/ab.err"
done
