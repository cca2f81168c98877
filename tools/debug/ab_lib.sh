# A/B two builds of the library on one box: tools/debug/ab_lib.sh <alt .so name under csrc/alt> [bench args...]
# Writes ab_{base,alt}_<rep>.json and ab.err into $OUT (default bench_out/).
set -e
ALT=$1; shift
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for rep in 1 2; do
  python bench.py --full --no-cpu-baseline --steps 64 --warmup 8 --no-prefill-timing "$@" > "$OUT/ab_base_$rep.json" 2>> "$OUT/ab.err"
  MLX_PARALLM_AMD_LIB=$PWD/mlx_parallm_amd/csrc/alt/$ALT python bench.py --full --no-cpu-baseline --steps 64 --warmup 8 --no-prefill-timing "$@" > "$OUT/ab_alt_$rep.json" 2>> "$OUT/ab.err"
done
