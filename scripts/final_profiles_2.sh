set -x
TAG=${1:-r04}
export PROFILE_OUT=${PROFILE_OUT:-profile_out}      # where the runs below write (created if missing)
mkdir -p $PROFILE_OUT
bash scripts/profile_bench.sh ${TAG}_cfg3 cfg3 > $PROFILE_OUT/prof_${TAG}_cfg3.log 2>&1
bash scripts/profile_bench.sh ${TAG}_cfg5 cfg5 > $PROFILE_OUT/prof_${TAG}_cfg5.log 2>&1
python bench.py --configs 1,2,3,4,4b,5 --steps 10 --cfg-cpu-units 2 > $PROFILE_OUT/${TAG}_configs.jsonl 2> $PROFILE_OUT/${TAG}_configs.err
cut -c1-300 $PROFILE_OUT/${TAG}_configs.jsonl
