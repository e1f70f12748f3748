#!/bin/bash
# Parent against new library in alternating processes of one session (MI355X). P: a checkout of the
# parent commit with its library built (default ab/parent); the new tree is the current directory.
# Usage: profiles/quiet_batch/ab.sh stretch|trace|abba|configs   (results under $OUT, default prof_out/quiet_batch)
# Every GPU step runs under its own time limit and the script stops at the first that fails.
set -e -o pipefail
export TMPDIR=${TMPDIR:-/tmp}
N=$(pwd)
P=$(cd "${P:-ab/parent}" && pwd)
O=${OUT:-prof_out/quiet_batch}
mkdir -p "$O"
O=$(cd "$O" && pwd)
Q=$N/profiles/quiet_batch
run() { (cd "$1" && shift && timeout -k 10 "$@"); }  # run TREE SECONDS command...
case "$1" in
stretch)  # rounds 102..301: three runs each of parent, new, new with a launch per round
  for i in 1 2 3; do
    run "$P" 120 python "$Q/stretch.py" parent >> "$O/launches.jsonl"
    run "$N" 120 python "$Q/stretch.py" new >> "$O/launches.jsonl"
    GX_QUIET_BATCH=1 run "$N" 120 python "$Q/stretch.py" new_batch1 >> "$O/launches.jsonl"
  done
  ;;
trace)  # kernel trace of the plain bench (nothing else traced), then the outputs file by file
  for t in parent new; do
    [ $t = parent ] && T=$P || T=$N
    rm -rf "$O/trace_$t" && mkdir -p "$O/trace_$t"
    run "$T" 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace_$t" -o run -- python bench.py --steps 100 --warmup 2 > "$O/trace_$t/bench.json"
    python "$Q/trace_sum.py" $t "$(find "$O/trace_$t" -name 'run_kernel_trace.csv' | head -1)" >> "$O/trace_sum.jsonl"
    run "$T" 240 python bench.py --steps 100 --warmup 2 --dump-outputs "$O/dump_$t" > /dev/null
  done
  (cd "$O" && for f in $(ls dump_parent); do cmp -s dump_parent/$f dump_new/$f && echo "$f identical" || echo "$f DIFFERS"; done) > "$O/dump_cmp.txt"
  ;;
abba)  # plain bench.py, P N N P, three times
  for i in 1 2 3; do
    for t in parent new new parent; do
      [ $t = parent ] && T=$P || T=$N
      run "$T" 240 python bench.py | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(json.dumps({'lib': '$t', 'rep': $i, 'value': d.get('value'), 'ms_per_step': d.get('ms_per_step')}))" >> "$O/abba_bench.jsonl"
    done
  done
  ;;
configs)  # the configs with few or no quiet rounds, interleaved, REPS runs each (the order swaps with every repeat)
  for i in $(seq 1 ${REPS:-2}); do
    for c in ${CONFIGS:-cfg2 cfg3 cfg4}; do
      for t in $([ $((i % 2)) = 1 ] && echo parent new || echo new parent); do
        [ $t = parent ] && T=$P || T=$N
        run "$T" 240 python bench.py --config $c | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(json.dumps({'lib': '$t', 'config': '$c', 'rep': $i, 'value': d.get('value'), 'ms_per_step': d.get('ms_per_step')}))" >> "$O/other_configs.jsonl"
      done
    done
  done
  ;;
*) echo "usage: $0 stretch|trace|abba|configs" >&2; exit 2 ;;
esac
