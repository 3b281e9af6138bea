set -x
export OUT=${OUT:-build/logs}     # output directory (git-ignored)
mkdir -p $OUT
rocminfo | grep -E "Marketing Name|gfx9|Compute Unit" | head -6 > $OUT/rocminfo.txt
nproc >> $OUT/rocminfo.txt; lscpu | grep "Model name" >> $OUT/rocminfo.txt
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke rc=$?" >> $OUT/smoke.log
timeout 1500 python -m pytest tests -m gpu -q ${PYTEST_EXTRA:-} 2>&1 | grep -vE "^layerInd|^\[INFO\]|^\[CHECK" > $OUT/pytest_gpu.log
timeout 900 python bench.py --full --steps 5 --warmup 2 > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?" >> $OUT/bench.err
tail -5 $OUT/smoke.log; tail -30 $OUT/pytest_gpu.log; cat $OUT/bench.json; tail -5 $OUT/bench.err
