# GPU box: the group kernel's block-size cap (VTMHIP_TZ_GROUP_ITEMS) on the quadtree and the split-shape partitions.  usage: gpurun -- 'bash scripts/gpu_group_items.sh'
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p "$OUT"      # where the bench lines and logs go
for it in 16 32; do for part in qt btt; do
VTMHIP_TZ_GROUP_ITEMS=$it timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 20 --partition $part > $OUT/gi.json 2> $OUT/gi.err || { tail -3 $OUT/gi.err; exit 1; }
python -c "
import json; d=json.load(open('$OUT/gi.json')); print('items $it $part', round(d['ms_per_step'],3), {k: round(v['ms_per_step'],3) for k,v in d['kernels'].items() if 'tz_' in k})"
done; done
