# Round-end evidence, short form (one pass of the GPU suite): suite, smoke, bench, kernel statistics and a one-step
# timeline of the same bench command.  Outputs under $OUT_DIR (default out/).
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${OUT_DIR:-out}
mkdir -p $out
timeout -k 10 400 python -m pytest tests -q -m gpu > $out/final_tests.log 2>&1 || { tail -30 $out/final_tests.log; exit 1; }
tail -1 $out/final_tests.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
python bench.py --full 2>/dev/null | tail -1 > $out/final_bench.json
rm -rf $out/prof_final
rocprofv3 --kernel-trace --stats -d $out/prof_final -- python3 bench.py --profile-only --steps 5 --warmup 2 > $out/prof_final.log 2>&1
python tools/step_timeline.py $out/prof_final > $out/final_timeline.txt 2>&1 || true
python tools/kernel_stats.py $out/prof_final > $out/final_kernel_stats.csv
rm -rf $out/prof_final
head -c 300 $out/final_bench.json; echo
python -c "
import json;d=json.load(open('$out/final_bench.json'));print(json.dumps(d['head_gemm']))"
