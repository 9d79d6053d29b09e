OUT=${OUT:-bench_out}
mkdir -p "$OUT"
run() { name=$1; shift; env "$@" python bench.py --full --no-cpu-baseline --no-tree-only --steps 30 > "$OUT/ab_$name.json" 2> "$OUT/ab_$name.err"; python -c "
import json,sys; d=json.load(open('$OUT/ab_$name.json')); print('$name', d['value'], d['backprop_kernel_avg_us'], d['roofline']['avg_launch_us'])"; }
