set -x
# The headline workload's profiles after a change that leaves the kernels alone (host-side symbolic / ordering): kernel stats and the
# three counter passes (scripts/profile_bench.sh), the traffic summary installed on the box, then the default bench line measured
# against it and the step timeline.  scripts/final_profiles_1.sh / _2.sh remain the full set.
TAG=${1:-r04}
export PROFILE_OUT=${PROFILE_OUT:-profile_out}      # where the runs below write (created if missing)
mkdir -p $PROFILE_OUT
bash scripts/profile_bench.sh ${TAG} > $PROFILE_OUT/prof_${TAG}.log 2>&1 || exit 1
python scripts/summarize_profile.py $PROFILE_OUT/profile_${TAG} profiles ${TAG} > /dev/null || exit 1
python bench.py --full > $PROFILE_OUT/bench_${TAG}_default.json 2> $PROFILE_OUT/bench_${TAG}_default.err || exit 1
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --output-format csv -d $PROFILE_OUT/prof_trace_${TAG} -- python3 bench.py --steps 3 --warmup 2 --no-cpu-baseline --no-scale-modes > $PROFILE_OUT/trace_${TAG}.log 2>&1 || exit 1
python scripts/step_timeline.py $PROFILE_OUT/prof_trace_${TAG} 3 > $PROFILE_OUT/${TAG}_step_timeline.txt
python scripts/bench_system.py > $PROFILE_OUT/${TAG}_system.json 2> $PROFILE_OUT/${TAG}_system.err
cut -c1-400 $PROFILE_OUT/bench_${TAG}_default.json
