#!/bin/bash
# The fused attention-propagation MLP launches (pk_attn_mlp_fwd / _bwd_norm / _bwd_in,
# PK_ATTN_MLP_FUSE=1) against the per-layer launches (PK_ATTN_MLP_FUSE=0) in the overlapped training
# and inference steps, alternating runs on one box, unprofiled. Each run has its own time limit; the
# script stops at the first run that fails.
#   bash tools/attn_mlp_ab.sh OUTPUT_DIR [REPS] [VARIANTS]      (VARIANTS e.g. "0 1 fwd bwd")
export TMPDIR=/tmp
O=${1:?usage: attn_mlp_ab.sh OUTPUT_DIR [REPS] [VARIANTS]}
REPS=${2:-3}
VARIANTS=${3:-"0 1"}
mkdir -p $O
i=0
for rep in $(seq 1 $REPS); do
  for mode in train infer; do
    for v in $VARIANTS; do
      i=$((i+1))
      PK_ATTN_MLP_FUSE=$v timeout -k 10 200 python bench.py --mode $mode --steps 30 --warmup 5 --no-cpu-baseline --no-roofline-probe --probe-steps 0 > $O/b_$i.log 2>&1 || { tail -20 $O/b_$i.log; exit 1; }
      grep "^{\"metric\"" $O/b_$i.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('$mode fuse=$v rep=$rep', d['value'], d['ms_per_step'])" | tee -a $O/ab.txt
    done
  done
done
