# GPU box: parity tests on the tree's library, then its bench beside prebuilt variants vtm_amd/libvtmhip_<tag>.so (bench only: no tests on the variants).
# usage: gpurun -- 'bash scripts/gpu_ab_lib.sh "<pytest files>" "<kernel substring>" tag1 tag2 ...'
set -e
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p "$OUT"      # where the bench lines and logs go
TESTS=$1; K=$2; shift; shift
timeout -k 10 700 python -m pytest $TESTS -m gpu -x -q > $OUT/ab_tests.log 2>&1 || (grep -n "^E " $OUT/ab_tests.log | head -20; tail -5 $OUT/ab_tests.log; exit 1)
tail -1 $OUT/ab_tests.log
cp vtm_amd/libvtmhip.so /tmp/libvtmhip_orig.so
trap 'cp /tmp/libvtmhip_orig.so vtm_amd/libvtmhip.so' EXIT
for t in tree "$@"; do
  if [ $t != tree ]; then cp vtm_amd/libvtmhip_$t.so vtm_amd/libvtmhip.so; fi
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 20 > $OUT/ab_${t}.json 2> $OUT/ab_${t}.err || (tail -5 $OUT/ab_${t}.err; exit 1)
  python - <<PY
import json
d = json.load(open("$OUT/ab_${t}.json"))
print("${t}", round(d["ms_per_step"], 3), {k: round(v["ms_per_step"], 3) for k, v in d["kernels"].items() if "$K" in k}, {k: round(v, 3) for k, v in d["stages_ms"].items()})
PY
done
