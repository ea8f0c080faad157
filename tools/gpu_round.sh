#!/bin/bash
# one gpurun call: GPU tests, a default bench run, a kernel-trace profile of a short bench run
# usage (on the GPU box, from the repo root): [OUT=dir] tools/gpu_round.sh TAG [pytest -k expr]   (results: ${OUT:-runs}/TAG/)
TAG=${1:-r02_a}
KEXPR=${2:-}
export TMPDIR=/tmp
O=${OUT:-runs}/$TAG
mkdir -p $O
if [ -n "$KEXPR" ]; then
  timeout 1500 python -m pytest tests -m gpu -q -x -k "$KEXPR" -s > $O/pytest.log 2>&1
else
  timeout 1500 python -m pytest tests -m gpu -q -s > $O/pytest.log 2>&1
fi
echo "pytest rc=$?" >> $O/pytest.log
tail -5 $O/pytest.log
timeout 600 python bench.py --full > $O/bench.json 2> $O/bench.err
echo "bench rc=$?"; tail -c 3000 $O/bench.json
timeout 600 python bench.py --steps 20 --warmup 5 > $O/bench_driver_args.json 2>> $O/bench.err
root=$(pwd); p=$(mktemp -d)
(cd $p && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $p/prof -o p -- python $root/bench.py --full --steps 100 --warmup 10 --cpu-steps 0 --parity 0 --fp32-leg 0 --np-steps 0 > $p/prof.log 2>&1)
f=$(find $p/prof -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && python tools/summarize_rocprof.py $f $O/kernel_stats.md "$TAG: bench.py --full --steps 100 --warmup 10 (default config)"
grep -h "^{" $p/prof.log > $O/bench_under_rocprof.json
