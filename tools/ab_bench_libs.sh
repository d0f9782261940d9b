#!/bin/bash
# Parent and child alternated in ONE process tree, whole bench.py processes: tools/ab_bench_libs.sh CONFIG PAIRS OUTFILE [STEPS]
#   parent: jolideco_amd/libjolideco_hip_parent.so (make -C jolideco_amd/csrc VARIANT=parent in a checkout of the parent
#           commit, the .so copied here), run through tools/bench_old_library.py -- the parent's LIBRARY under this tree's
#           Python;  child: the in-tree build, plain bench.py
#   PARENT_CHECKOUT=DIR: the parent arm is plain bench.py run inside DIR instead, a whole checkout of the parent commit with
#           its library built in-tree -- its Python AND its library, for a change that moves work between the two
#   STEPS: bench.py's --steps (default 200; c6 runs a tenth of it per region, so 2000 there gives regions of 200 steps)
# Every run is `bench.py --gpus 1 --config CONFIG --repeats 9` under its own time limit; OUTFILE receives bench.py's result
# line of every run behind "pair N parent|child"; the first failure ends the script.
set -o pipefail
CFG=$1; PAIRS=$2; OUT=$(realpath -m "$3"); STEPS=${4:-200}
ROOT=$(pwd)
: > "$OUT"
ONE=$(mktemp)
for p in $(seq 1 "$PAIRS"); do
  for lib in parent child; do
    if [ $lib = child ]; then
      timeout -k 10 240 python bench.py --gpus 1 --config "$CFG" --repeats 9 --steps "$STEPS" > "$ONE" 2> "$ONE.err"
    elif [ -n "$PARENT_CHECKOUT" ]; then
      (cd "$PARENT_CHECKOUT" && timeout -k 10 240 python bench.py --gpus 1 --config "$CFG" --repeats 9 --steps "$STEPS") > "$ONE" 2> "$ONE.err"
    else
      JOLIDECO_HIP_LIBRARY=jolideco_amd/libjolideco_hip_parent.so timeout -k 10 240 python tools/bench_old_library.py --gpus 1 --config "$CFG" --repeats 9 --steps "$STEPS" > "$ONE" 2> "$ONE.err"
    fi
    rc=$?
    cd "$ROOT"
    if [ $rc -ne 0 ]; then echo "pair $p $lib FAILED with $rc" | tee -a "$OUT"; tail -n 20 "$ONE.err"; exit $rc; fi
    echo "pair $p $lib $(grep '^{' "$ONE" | tail -n 1)" >> "$OUT"
    tail -n 1 "$OUT" | grep -o 'pair [0-9]* [a-z]*\|"ms_per_step[a-z_]*": [0-9.]*' | tr '\n' ' '; echo
  done
done
rm -f "$ONE" "$ONE.err"
