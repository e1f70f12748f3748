#!/bin/bash
# Sharded probe_piggyback at G = 8, cfg 5, rounds 51-59 on one GPU:
#   1. probes off, the parent commit's build ($1) against this one, alternating in one process;
#   2. probes on: the shard's round time and the plan's padding (slots planned / filled);
#   3. probes on under a kernel trace: each kernel's share of the shard's round.
# usage: profiles/probe_shards/run.sh <libgx of the parent commit> [output directory]
set -e -o pipefail
PARENT=$1
O=${2:-prof_out/probe_shards}
mkdir -p $O
timeout -k 10 600 python -u profiles/probe_shards/shard_probe_ab.py --libs $PARENT sidecar_amd/libgx.so --reps 3 \
  --out $O/ab_probes_off.jsonl
timeout -k 10 300 python -u profiles/probe_shards/shard_probe_ab.py --libs sidecar_amd/libgx.so --probe 1 --fill --reps 2 \
  --out $O/probes_on.jsonl
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/trace -o run -- python -u profiles/probe_shards/shard_probe_ab.py \
  --libs sidecar_amd/libgx.so --probe 1 --reps 1 > $O/trace.out 2>&1
python profiles/probe_shards/trace_rounds.py $O/trace/run_results.db > $O/probes_on_kernels_rounds_51_59.json
