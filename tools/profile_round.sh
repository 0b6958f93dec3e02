# The round's measurement record (argument: tag): the driver's bench command, then the same command
# under rocprofv3 --kernel-trace --stats (its kernel stats and its own bench line), into $OUT/
# for copying to profiles/.
set -e
cd "${GRAFT_REPO_ROOT:-/root/repo}"
OUT=${MMT_OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-run}
timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -20 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
rm -rf $OUT/prof_$TAG
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python bench.py --full > $OUT/bench_${TAG}_under_rocprof.json 2> $OUT/bench_${TAG}_under_rocprof.err
python tools/rocprof_summary.py $OUT/prof_$TAG $OUT/kernel_stats_$TAG.csv | grep mmt | head -25
rm -rf $OUT/prof_$TAG
