#!/bin/bash
# GPU box: everything profiles/r03_* is made of.  Output under gpurun_out/r03/ (+ gpurun_out/prof, prof_sq), summarised by
# tools/summarize_profiles.py / tools/summarize_sq.py here in the build container.   gpurun -- 'bash tools/collect_r03.sh [quick]'
export TMPDIR=/tmp
R=$PWD/gpurun_out/r03; rm -rf $R; mkdir -p $R
python bench.py --full --steps 20 --warmup 3 > $R/bench_default.json 2> $R/bench_default.err
python bench.py --full --steps 20 --warmup 3 --no-cpu --batch 16384 > $R/bench_16k.json 2>/dev/null
# the same sources with the compiler's default code generation for the solver kernel (lib_defaultflags.so, built by build())
FRP_LIB=$PWD/forces_resilient_planner_amd/lib_defaultflags.so python bench.py --full --steps 20 --warmup 3 --no-cpu > $R/bench_defaultflags.json 2>/dev/null
# the other BASELINE configs and the strong-scaling form (RCCL world 1)
for c in "--config 3" "--config 3 --scaling strong" "--config 4" "--config 2 --scaling strong"; do
  FRP_BENCH_FORCE_DIST=$([[ "$c" == *strong* ]] && echo 1) python bench.py --full --steps 10 --warmup 2 --repeats 3 --no-cpu $c 2>/dev/null | tail -1 >> $R/other_configs.jsonl
done
python tools/bench_configs.py > $R/bench_configs.txt 2>&1
if [ -f forces_resilient_planner_amd/lib_prof.so ]; then
  for b in 1 4096; do FRP_LIB=$PWD/forces_resilient_planner_amd/lib_prof.so python tools/prof_lds.py $b 2 >> $R/wave_phases.txt 2>&1; done
fi
timeout 60 tools/ubench/sweep_timing > $R/sweep_timing.txt 2>&1
python tests/tools/e2e_bench.py > $R/e2e.txt 2>/dev/null
python tools/order_ceiling.py 4096 > $R/order_ceiling.jsonl 2>/dev/null; python tools/order_ceiling.py 16384 >> $R/order_ceiling.jsonl 2>/dev/null
bash tools/ab_order.sh > $R/order_weights.txt 2>&1
python tools/full_tick_bench.py 4096 10 20000 > $R/full_tick.json 2> $R/full_tick.err
python tools/receding_bench.py 65536 20 > $R/configs4_receding.json 2>/dev/null
python tests/tools/astar_bench.py 1024 pillars 20000 2>/dev/null | tail -1 > $R/astar_bench.jsonl
python tests/tools/astar_bench.py 4096 empty 4000 2>/dev/null | tail -1 >> $R/astar_bench.jsonl
python tests/tools/astar_bench.py 1024 wall_gap 20000 2>/dev/null | tail -1 >> $R/astar_bench.jsonl
python tests/tools/astar_check.py 12 16 > $R/astar_check.txt 2>&1
if [ "$1" != "quick" ]; then
  python tests/tools/sweep_check.py > $R/sweep_check.txt 2>&1
  python tests/tools/soak.py 240 > $R/soak.txt 2>&1
fi
bash tools/collect_profiles.sh > $R/collect_profiles.log 2>&1
bash tools/collect_sq_counters.sh > $R/collect_sq.log 2>&1
ls $R
