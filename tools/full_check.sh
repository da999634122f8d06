cd "$(dirname "$0")/.."; O=${OUT_DIR:-check_out}; mkdir -p $O
timeout 2400 python -m pytest tests -m gpu -x -q > $O/r4c_pytest.log 2>&1; echo "pytest rc=$?"; tail -3 $O/r4c_pytest.log
python bench.py --full > $O/r4c_bench.json 2> $O/r4c_bench.err; O=$O python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ['O'], 'r4c_bench.json')).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline']['frac'], d.get('cpu_baseline',{}).get('value'))
PY
