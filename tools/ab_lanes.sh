OUT=${1:?usage: bash tools/ab_lanes.sh <output dir>}
mkdir -p $OUT
python -m pytest tests/test_train_gpu.py -x -q -m gpu -k "wgrad_lanes" > $OUT/pytest.log 2>&1; echo "pytest rc=$?"; tail -5 $OUT/pytest.log
for v in 0 1 0 1; do
  python bench.py --full --steps 30 --warmup 8 --no-cpu-baseline --wgrad-lanes $v > $OUT/c2_l$v.json 2> $OUT/c2_l$v.err
  python -c "import json; d=json.load(open('$OUT/c2_l$v.json')); print('C2 lanes=$v', d['value'], d['ms_per_step'], d.get('windows_ms_per_step'), d.get('host_enqueue_ms_per_step'))"
done
for v in 0 1; do
  python bench.py --full --steps 30 --warmup 8 --no-cpu-baseline --graph --wgrad-lanes $v > $OUT/c2g_l$v.json 2> $OUT/c2g_l$v.err
  python -c "import json; d=json.load(open('$OUT/c2g_l$v.json')); print('C2 graph lanes=$v', d['value'], d['ms_per_step'], d.get('windows_ms_per_step'))"
done
for v in 0 1; do
  python bench.py --full --steps 15 --warmup 5 --no-cpu-baseline --batch 8 --height 320 --width 1024 --num-layers 50 --wgrad-lanes $v > $OUT/c3_l$v.json 2> $OUT/c3_l$v.err
  python -c "import json; d=json.load(open('$OUT/c3_l$v.json')); print('C3 lanes=$v', d['value'], d['ms_per_step'], d.get('windows_ms_per_step'))"
done
python tools/sweep_g1wgrad.py > $OUT/sweep_g1w.txt 2>&1; tail -3 $OUT/sweep_g1w.txt
