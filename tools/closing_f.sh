# tools/closing_f.sh -- after bench.py's legs were reordered (fixed-base leg before the headline): the bench-contract tests, the driver's
# command, the same command's MSM legs under rocprofv3 (kernel stats + the line printed under the profiler), the two-rank rehearsal.
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
T=r05_f
OUT=${OUT:-out}; mkdir -p $OUT        # where the outputs go
timeout -k 10 500 python3 -m pytest tests/test_bench_contract_gpu.py -x -q -m gpu > $OUT/${T}_contract.log 2>&1 || { tail -30 $OUT/${T}_contract.log; exit 1; }
echo "contract tests done"; tail -2 $OUT/${T}_contract.log
timeout -k 10 400 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${T}_bench.json 2> $OUT/${T}_bench.err || { tail -20 $OUT/${T}_bench.err; exit 1; }
echo "bench done"
mkdir -p $OUT/${T}_h
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${T}_h -- python3 bench.py --full --steps 20 --warmup 5 --no-plonk --no-ntt --no-cpu-baseline --no-batch > $OUT/${T}_bench_headline_under_rocprof.json 2> $OUT/${T}_h/err.txt || { tail -20 $OUT/${T}_h/err.txt; exit 1; }
cp "$(find $OUT/${T}_h -name '*kernel_stats.csv' | head -1)" $OUT/${T}_bench_headline_kernel_stats.csv
find $OUT/${T}_h -name '*kernel_trace.csv' -delete
echo "headline profile done"
python3 - <<P
import json
for f in ("$OUT/${T}_bench.json", "$OUT/${T}_bench_headline_under_rocprof.json"):
    d = json.loads(open(f).read().strip().splitlines()[-1])
    print(f, "step %.3f ms" % d["ms_per_step"], "acc", d["roofline"]["avg_launch_ms"], d["phases_ms"], "| fixed-base %.3f" % d["fixed_base"]["ms_per_step"], d["config"]["leg_order"][:40])
P
bash tools/rehearse_two_ranks.sh $T
