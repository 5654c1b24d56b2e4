# The full bench line (bench.py --full) and a rocprofv3 --kernel-trace --stats summary of the same run's kernels.  usage: bash scripts/prof_loop.sh [out dir]
R=$(cd "$(dirname "$0")/.." && pwd); O=${1:-/tmp/prof_loop_out}; mkdir -p $O; O=$(cd $O && pwd)
cd /tmp && export TMPDIR=/tmp
python $R/bench.py --full --cpu-steps 0 --no-learner-only > $O/bench_now.json 2>/dev/null
rm -rf /tmp/prof_loop
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_loop -- python $R/bench.py --full --steps 100 --warmup 20 --cpu-steps 0 --no-learner-only > /tmp/prof_loop.log 2>&1
f=$(find /tmp/prof_loop -name "*kernel_stats.csv" | head -1)
python $R/scripts/prof_summary.py $f 14 > $O/prof_loop_split.txt
cat $O/prof_loop_split.txt
python -c "
import json; d=json.load(open('$O/bench_now.json')); print('bench', d['value'], d['ms_per_step'], d['roofline']['launch_ms'], d['roofline']['frac'])"
