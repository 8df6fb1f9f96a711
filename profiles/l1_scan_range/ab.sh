#!/bin/bash
# A/B against the parent commit on one box: PARENT = a built checkout of the parent commit, run from the root of a built
# checkout of this one.  `ab.sh` : parent, new, parent, new ... three each of the six bench lines, then the two kernel traces.
#                        `ab.sh half` : the two half-precision lines, five pairs, parent and new back to back.
# Every GPU step runs under its own time limit and the script ENDS at the first one that fails (a fault, an abort, a time
# limit): nothing more is started on that card.
set -o pipefail
PARENT=${PARENT:?path of a built checkout of the parent commit}
ROOT=$(pwd); OUT=${OUT:-$(mktemp -d)}; mkdir -p $OUT; echo "results in $OUT"
export MDK_SKIP_BUILD=1
run() {  # tree name bench-arguments...
  local tree=$1 name=$2; shift 2
  local dir=$ROOT; [ $tree = parent ] && dir=$PARENT
  ( cd $dir && timeout -k 10 150 python bench.py --gpus 1 --steps 20 --warmup 5 "$@" 2>>$OUT/${tree}_${name}.err | tail -1 >> $OUT/${tree}_${name}.jsonl )
  local rc=$?      # (pipefail: bench.py's status, not tail's)
  if [ $rc -ne 0 ]; then echo "$tree $name: bench.py ended with status $rc -- stopping here"; tail -5 $OUT/${tree}_${name}.err; exit $rc; fi
}
if [ "$1" = half ]; then
  for rep in 1 2 3 4 5; do
    for tree in parent new; do run $tree half --half; done
    for tree in new parent; do run $tree devonly_half --device-only --half; done
  done
  python profiles/l1_scan_range/ab_table.py $OUT
  exit $?
fi
for rep in 1 2 3; do
  for tree in parent new; do
    run $tree headline
    run $tree batch100 --batch 100
    run $tree half --half
    run $tree devonly --device-only
    run $tree devonly_b100 --device-only --batch 100
    run $tree devonly_half --device-only --half
  done
done
python profiles/l1_scan_range/ab_table.py $OUT || exit 1
# kernel evidence, parent then new: the second only if the first ended well
( cd $PARENT && timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $OUT/trace_parent -o parent --output-format csv -- python bench.py --device-only --steps 10 ) &&
  timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $OUT/trace_new -o new --output-format csv -- python bench.py --device-only --steps 10
rc=$?
[ $rc -eq 0 ] || echo "kernel trace ended with status $rc"
exit $rc
