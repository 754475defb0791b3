#!/bin/bash
# Everything profiles/ holds for a round, in one go on the MI355X box (from the repository root):
#   scripts/profile_round.sh r02 [particles]
# bench line (--full), rocprofv3 kernel stats of the same command, fabric traffic (PMC), SQ counters.  Outputs land in
# $SC_PROFILE_OUT/<tag>_* (default profile_out/); copy what is to be judged into profiles/.
export TMPDIR=/tmp
TAG=${1:-r04}
export SC_PROFILE_TAG=$TAG
N=${2:-1048576}
OUT=${SC_PROFILE_OUT:-profile_out}
mkdir -p $OUT
python bench.py --full --particles $N > $OUT/${TAG}_bench_$N.json 2> $OUT/${TAG}_bench_$N.err || tail -5 $OUT/${TAG}_bench_$N.err
# the kernel trace three times over (the boxes of the pool differ by ~2 %, and so do cold-clock runs on one box); the
# run with the median pair time is the one that is kept, the three pair times are listed next to it
for k in 1 2 3; do
  rm -rf $OUT/${TAG}_stats_${N}_$k
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stats_${N}_$k -- python bench.py --particles $N --cpu-sample 0 --no-kernel-events --repeats 1 --clock-warmup 0 > $OUT/${TAG}_stats_${N}_$k.log 2>&1 || tail -5 $OUT/${TAG}_stats_${N}_$k.log
  # per-call durations of the workload's launches only (the --stats CSV averages the primer's launches in): what
  # bench.py reports as roofline.rocprof
  python scripts/summarize_trace.py $OUT/${TAG}_stats_${N}_$k $OUT/${TAG}_kernel_calls_${N}_$k.json $N > $OUT/${TAG}_kernel_calls_${N}_$k.log 2>&1 || tail -3 $OUT/${TAG}_kernel_calls_${N}_$k.log
done
MED=$(python - <<PY
import json
runs = [(json.load(open(f"$OUT/${TAG}_kernel_calls_${N}_{k}.json"))["pair"]["avg_launch_us"], k) for k in (1, 2, 3)]
runs.sort()
k = runs[1][1]
d = json.load(open(f"$OUT/${TAG}_kernel_calls_${N}_{k}.json"))
d["pair"]["three_runs_avg_launch_us"] = [r[0] for r in runs]
d["pair"]["kept"] = "the run with the median pair time"
json.dump(d, open("$OUT/${TAG}_kernel_calls_${N}.json", "w"), indent=1)
print(k)
PY
)
cp $OUT/${TAG}_stats_${N}_$MED/*/*kernel_stats.csv $OUT/${TAG}_kernel_stats_$N.csv 2>/dev/null
# the raw per-dispatch trace of the same run (~50 KB gzipped): the per-call summary can be re-derived from it
gzip -c $OUT/${TAG}_stats_${N}_$MED/*/*kernel_trace.csv > $OUT/${TAG}_kernel_trace_$N.csv.gz 2>/dev/null
cp $OUT/${TAG}_kernel_calls_${N}_$MED.log $OUT/${TAG}_kernel_calls_$N.log
scripts/collect_traffic.sh $N > $OUT/${TAG}_traffic_$N.log 2>&1 || tail -5 $OUT/${TAG}_traffic_$N.log
cp profiles/${TAG}_traffic_$N.json $OUT/ 2>/dev/null
scripts/collect_sq.sh $N > $OUT/${TAG}_sq_$N.log 2>&1 || tail -5 $OUT/${TAG}_sq_$N.log
cp profiles/${TAG}_sq_$N.json $OUT/ 2>/dev/null
tail -c 600 $OUT/${TAG}_bench_$N.json; echo; tail -14 $OUT/${TAG}_kernel_calls_$N.log; tail -12 $OUT/${TAG}_traffic_$N.log; tail -8 $OUT/${TAG}_sq_$N.log
