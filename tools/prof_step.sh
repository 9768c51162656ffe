# Kernel statistics + one-step timeline of the large-batch bench step: tools/prof_step.sh <tag> [ENV=VAL ...]
# (BENCH_ARGS="--storage bf16" etc. are passed to bench.py)
# -> $OUT_DIR (default out/): <tag>_bench.json, <tag>_kernel_stats.csv, <tag>_timeline.txt
set -e
tag=$1; shift
for kv in "$@"; do export "$kv"; done
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${OUT_DIR:-out}
mkdir -p $out
python bench.py --full --profile-only --steps 20 --warmup 3 ${BENCH_ARGS} 2>/dev/null | tail -1 > $out/${tag}_bench.json
rm -rf $out/prof_$tag
rocprofv3 --kernel-trace --stats -d $out/prof_$tag -- python3 bench.py --profile-only --steps 5 --warmup 2 ${BENCH_ARGS} > $out/prof_$tag.log 2>&1
python tools/step_timeline.py $out/prof_$tag > $out/${tag}_timeline.txt 2>&1 || true
python tools/kernel_stats.py $out/prof_$tag > $out/${tag}_kernel_stats.csv
rm -rf $out/prof_$tag
python -c "
import json,sys
d=json.loads(open('$out/${tag}_bench.json').read())
print('$tag', d['value'], d['ms_per_step'])"
