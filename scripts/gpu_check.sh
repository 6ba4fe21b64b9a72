# GPU box: parity tests + a short bench line.  usage: gpurun -- 'bash scripts/gpu_check.sh'
set -e
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p "$OUT"      # where the bench lines and logs go
python -m pytest tests -m gpu -q -x > $OUT/pl.txt 2>&1 || (grep -n "^E " $OUT/pl.txt | head -20; tail -5 $OUT/pl.txt; exit 1)
tail -2 $OUT/pl.txt
python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline 2>$OUT/bench_err.txt | tail -1 > $OUT/bench_tmp.json || (tail -30 $OUT/bench_err.txt; exit 1)
python -c "
import json; d=json.load(open('$OUT/bench_tmp.json')); print({k:d[k] for k in ('value','ms_per_step','satd_gblocks_per_s')}); print(d['stages_ms']); print(d['roofline'])"
