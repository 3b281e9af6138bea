# round 5, final: GPU tier, the driver's bench command, the rocprofv3 passes (profiles/r5_v11, profiles/r5_vgg16)
set -x
export OUT=${OUT:-build/logs}     # output directory (git-ignored)
mkdir -p $OUT/r5z
timeout 1800 python -m pytest tests -m gpu -q 2>&1 | grep -vE "^layerInd|^\[INFO\]|^\[CHECK" > $OUT/r5z/pytest_gpu.log
tail -6 $OUT/r5z/pytest_gpu.log | cut -c1-300
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/r5z/smoke.log 2>&1; tail -2 $OUT/r5z/smoke.log
timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/r5z/bench.json 2> $OUT/r5z/bench.err; echo "bench rc=$?" >> $OUT/r5z/bench.err
tail -3 $OUT/r5z/bench.err
bash scripts/gpu_prof.sh > $OUT/prof.log 2>&1
bash scripts/gpu_prof_vgg.sh > $OUT/prof_vgg.log 2>&1
python - <<'P'
import json, os
b=json.loads(open(os.environ['OUT'] + '/r5z/bench.json').readline())
print({k:b[k] for k in b if k.startswith('value')})
print("parity", b['parity']['ok'], "vgg parity", b['vgg16']['parity']['ok'])
P
