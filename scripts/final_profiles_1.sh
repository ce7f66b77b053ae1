set -x
TAG=${1:-r04}
export PROFILE_OUT=${PROFILE_OUT:-profile_out}      # where the runs below write (created if missing)
mkdir -p $PROFILE_OUT
bash scripts/profile_bench.sh ${TAG} > $PROFILE_OUT/prof_${TAG}.log 2>&1
python bench.py --full > $PROFILE_OUT/bench_${TAG}_default.json 2> $PROFILE_OUT/bench_${TAG}_default.err
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --output-format csv -d $PROFILE_OUT/prof_trace_${TAG} -- python3 bench.py --steps 3 --warmup 2 --no-cpu-baseline --no-scale-modes > $PROFILE_OUT/trace_${TAG}.log 2>&1
python scripts/step_timeline.py $PROFILE_OUT/prof_trace_${TAG} 3 > $PROFILE_OUT/${TAG}_step_timeline.txt
python scripts/bench_system.py > $PROFILE_OUT/${TAG}_system.json 2> $PROFILE_OUT/${TAG}_system.err
python scripts/bench_multirhs.py --nrhs 1,8,16,64,512 --reps 7 > $PROFILE_OUT/${TAG}_multirhs.json 2> $PROFILE_OUT/${TAG}_multirhs.err
python bench.py --mode rhs --no-cpu-baseline > $PROFILE_OUT/${TAG}_bench_rhs.json 2> $PROFILE_OUT/${TAG}_bench_rhs.err
python bench.py --mode problems --no-cpu-baseline > $PROFILE_OUT/${TAG}_bench_problems.json 2> $PROFILE_OUT/${TAG}_bench_problems.err
bash scripts/hop_tables.sh ${TAG}
tail -c 400 $PROFILE_OUT/${TAG}_bench_rhs.json; tail -c 300 $PROFILE_OUT/${TAG}_bench_problems.json
