#!/bin/bash
# End-of-round validation on an MI355X: build check, GPU suite, smoke, the --full bench line (secondaries, CPU + eager baselines),
# and `python bench.py --gpus 2 --backend gloo` started WITHOUT a launcher (two ranks on the one GPU of the box)
O=gpurun_out/r4/final
mkdir -p $O
python -c "import __graft_entry__ as g; g.build()" > $O/build.log 2>&1; echo "build exit $?"
timeout 1500 python -m pytest tests -m gpu -q -s > $O/pytest_gpu_verbose.log 2>&1; echo "pytest exit $?"; tail -n 2 $O/pytest_gpu_verbose.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; echo "smoke exit $?"; tail -n 1 $O/smoke.log
timeout 1800 python bench.py --full > $O/bench.log 2> $O/bench.err; echo "bench exit $?"
timeout 600 python bench.py --gpus 2 --backend gloo --steps 2 --warmup 1 > $O/bench_2ranks_selfspawn.log 2>&1; echo "bench --gpus 2 (self-spawned, gloo) exit $?"; tail -n 1 $O/bench_2ranks_selfspawn.log | cut -c1-300
python - <<'PY'
import json
l=[x for x in open('gpurun_out/r4/final/bench.log') if x.startswith('{')][-1]
d=json.loads(l)
print('headline', round(d['value'],1), 'ms/step', round(d['ms_per_step'],1), 'kernel_ms', round(d['roofline']['kernel_ms'],1), 'frac', round(d['roofline']['frac'],4), d.get('value_by_noise_source'))
for s in d.get('secondary',[]):
    print(' ', s['tag'], s.get('compute_units_per_molecule'), round(s['molecules_per_s'],1), round(s['kernel_ms'] or 0,1), 'F_min frac', round(s['roofline_frac'],3), 'executed', round(s['executed_frac'],3))
print('cpu', d['cpu_baseline']['value'], d['cpu_baseline']['cores'])
print('eager', d['eager_rocm_baseline']['value'], d['eager_rocm_baseline']['ms_per_forward'])
PY
