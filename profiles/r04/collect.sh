# Collects the training-step evidence of this directory on the GPU machine:
#     [OUT=<directory>] bash profiles/r04/collect.sh <tag> [harness train-step arguments ...]      (OUT defaults to ./r04_out)
#   $OUT/<tag>_rep{1..5}.json   five repetitions of `python3 -m admm_net_amd.harness train-step --steps 30 <args>`
#   $OUT/<tag>_kernel_stats.csv one `rocprofv3 --kernel-trace --stats` run of `... --steps 5 <args>` (3 warm-up + 5 timed
#                                         steps = 8 optimisation steps), summarised by profiles/r04/summarize.py
#   $OUT/<tag>_trace.json       dispatches per step and the share of kernel time per class
# Tracing only, no counters; the program itself follows `--`.  Every step runs under its own time limit and the chain stops
# at the first failure.
set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
export TMPDIR=/tmp
TAG=$1; shift
OUT=${OUT:-r04_out}
mkdir -p $OUT
rm -rf $OUT/kt_$TAG
timeout -k 10 240 python3 -m admm_net_amd.harness train-step --steps 30 "$@" > $OUT/${TAG}_rep1.json &&
timeout -k 10 120 python3 -m admm_net_amd.harness train-step --steps 30 "$@" > $OUT/${TAG}_rep2.json &&
timeout -k 10 120 python3 -m admm_net_amd.harness train-step --steps 30 "$@" > $OUT/${TAG}_rep3.json &&
timeout -k 10 120 python3 -m admm_net_amd.harness train-step --steps 30 "$@" > $OUT/${TAG}_rep4.json &&
timeout -k 10 120 python3 -m admm_net_amd.harness train-step --steps 30 "$@" > $OUT/${TAG}_rep5.json &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/kt_$TAG -o $TAG -- python3 -m admm_net_amd.harness train-step --steps 5 "$@" > $OUT/${TAG}_rocprof_run.json 2> $OUT/${TAG}_rocprof.err &&
python3 profiles/r04/summarize.py $OUT/kt_$TAG $OUT/${TAG}_kernel_stats.csv 8 > $OUT/${TAG}_trace.json
rc=$?
cat $OUT/${TAG}_rep*.json $OUT/${TAG}_trace.json 2>/dev/null
find $OUT -name '*.db' -delete      # the trace databases (tens of MB) stay behind
rm -rf $OUT/kt_$TAG
echo "collect $TAG rc=$rc"
exit $rc
