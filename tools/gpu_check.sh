# pytest -m gpu + the full bench line + the all-reduce placement A/B at world size 1 (collective forced).
# Run from the repository root on a GPU node as: bash tools/gpu_check.sh OUTDIR   (logs and JSON lines land in OUTDIR)
OUT=${1:?usage: bash tools/gpu_check.sh OUTDIR}
mkdir -p $OUT
python -m pytest tests -m gpu -q --timeout 900 -x -s --durations=8 2>&1 | grep -v "^\.*$" | tail -150 > $OUT/pytest_gpu.log
tail -60 $OUT/pytest_gpu.log
python bench.py --steps 300 --warmup 30 --full 2> $OUT/bench_default.err | tail -1 > $OUT/bench_default.json
tail -5 $OUT/bench_default.err
OUT=$OUT python - <<'PY'
import json, os
d = json.load(open(os.path.join(os.environ['OUT'], 'bench_default.json')))
print('headline', round(d['value']), round(d['ms_per_step'] * 1e3, 1), 'us')
for k in ('module_surface', 'config3_emd', 'config5_progressive', 'batch_sweep', 'roofline_longest'):
    print(k, json.dumps(d.get(k))[:900])
PY
for mode in after graph graph-fork after graph graph-fork; do
  python bench.py --gpus 1 --force-collective --allreduce $mode --steps 1000 --warmup 50 --no-probes --full 2>$OUT/ar_$mode.err | tail -1 > $OUT/ar_$mode.json
  echo "allreduce=$mode $(cat $OUT/ar_$mode.json | head -c 300)"; tail -2 $OUT/ar_$mode.err
done
python bench.py --steps 1000 --warmup 50 --no-probes | tail -1
