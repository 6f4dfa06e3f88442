#!/bin/bash
# same-box A/B of library files over every bench leg: usage ab_full.sh <lib.so> <lib.so> ...
F=$(mktemp) && trap 'rm -f "$F"' EXIT || exit 1
for rep in 1 2; do
for lib in "$@"; do
  JACO_ENV_LIB=$lib timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 12 --warmup 3 2>/dev/null | tail -1 > "$F" || exit 1
  python tools/bench_summary.py "$F" | sed "s/^/$lib rep $rep: /"
done; done
