#!/bin/bash
# The block-MLP chain (pk_mlp3_fwd / pk_mlp3_bwd, PK_BLOCK_MLP_CHAIN=1) against the per-layer launches
# (PK_BLOCK_MLP_CHAIN=0) in the overlapped training and inference steps, alternating runs on one box,
# unprofiled.
#   bash tools/mlp_chain_ab.sh OUTPUT_DIR
export TMPDIR=/tmp
O=${1:?usage: mlp_chain_ab.sh OUTPUT_DIR}
mkdir -p $O
i=0
for rep in 1 2 3; do
  for mode in train infer; do
    for v in 0 1; do
      i=$((i+1))
      PK_BLOCK_MLP_CHAIN=$v timeout -k 10 200 python bench.py --mode $mode --steps 30 --warmup 5 --no-cpu-baseline --no-roofline-probe --probe-steps 0 > $O/b_$i.log 2>&1 || { tail -20 $O/b_$i.log; exit 1; }
      grep "^{\"metric\"" $O/b_$i.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('$mode chain=$v rep=$rep', d['value'], d['ms_per_step'])" | tee -a $O/ab.txt
    done
  done
done
