#!/bin/bash
# Hop timings of the persistent sweep kernel (1 and 2 columns) and of the chained launches: $PROFILE_OUT/<tag>_hops_*.txt
TAG=${1:-r04}
export PROFILE_OUT=${PROFILE_OUT:-profile_out}      # where the runs below write (created if missing)
mkdir -p $PROFILE_OUT
B="python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-scale-modes"
HIPKKT_CHAIN=0 HIPKKT_TOP_STAMPS=9 timeout -k 10 200 $B 2>&1 | grep "top stamps" > $PROFILE_OUT/${TAG}_hops_top_1col.txt
HIPKKT_CHAIN=0 HIPKKT_TOP_STAMPS=5 HIPKKT_TOP_STAMPS_NR=2 timeout -k 10 200 $B 2>&1 | grep "top stamps" > $PROFILE_OUT/${TAG}_hops_top_2col.txt
HIPKKT_TOP_STAMPS=9 timeout -k 10 200 $B 2>&1 | grep "chain stamps" > $PROFILE_OUT/${TAG}_hops_chain.txt
wc -l $PROFILE_OUT/${TAG}_hops_*.txt
