# Lean GPU pass: parity tests, smoke, bench, rocprofv3 kernel trace of the bench command (no PMC passes).
# usage (GPU box, repo root):  bash tools/gpu_lean.sh [tag] [extra pytest args]     (logs and trace land in profiles/<tag>/)
TAG=${1:-r1}
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$PWD}
O=$R/profiles/$TAG
mkdir -p $O
(timeout 900 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider 2>&1 | tail -40) > $O/pytest_gpu_$TAG.log 2>&1
(timeout 300 python __graft_entry__.py smoke 2>&1 | tail -5) > $O/smoke_$TAG.log 2>&1
(timeout 900 python bench.py --full --steps 1 --warmup 1 2>&1 | tail -5) > $O/bench_$TAG.log 2>&1
cd /tmp
(timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -o bench -- python $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline 2>&1 | tail -5) > $O/rocprof_$TAG.log 2>&1
cd $R
find $O -name "*.db" -delete 2>/dev/null
find $O -name "*kernel_trace.csv" -size +8M -exec gzip -f {} \;
tail -5 $O/pytest_gpu_$TAG.log; tail -2 $O/smoke_$TAG.log; tail -2 $O/bench_$TAG.log
