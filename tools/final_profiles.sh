#!/bin/bash
# Round-end measurement pass (on the GPU box): smoke, default bench line, T=9 / B=16 lines, rocprofv3 kernel stats (serial and fork/join
# schedules, fp32 and bf16 storage), timeline gaps of the replayed graph, PMC traffic passes, phase timeline, GEMM shape table,
# config-5 training lines.  Outputs under $MUMPY_PROFILE_OUT (default profile_out/; tag them into profiles/ with
# tools/collect_profiles.py).
export OMP_NUM_THREADS=${OMP_NUM_THREADS:-16}   # a box reports every host core; torch would start one thread per core
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
export MUMPY_PROFILE_OUT=${MUMPY_PROFILE_OUT:-$R/profile_out}
OUT=$MUMPY_PROFILE_OUT
mkdir -p $OUT
cd $R
python __graft_entry__.py smoke > $OUT/smoke.log 2>&1 || echo "SMOKE FAILED"
python bench.py --full > $OUT/bench_final.json 2> $OUT/bench_final.err || echo "BENCH FAILED"
echo "bench done"
python bench.py --full --frames 9 --no-cpu-baseline --no-alt > $OUT/bench_t9.json 2> $OUT/bench_t9.err || echo "BENCH T9 FAILED"
python bench.py --full --batch 16 --no-cpu-baseline --no-alt > $OUT/bench_b16.json 2> $OUT/bench_b16.err || echo "BENCH B16 FAILED"
python bench.py --full --batch 1 --no-cpu-baseline --no-alt > $OUT/bench_b1.json 2> $OUT/bench_b1.err || echo "BENCH B1 FAILED"
echo "bench variants done"
cd /tmp
MUMPY_SERIAL=1 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_serial -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-alt > $OUT/prof_serial.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_fj -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-alt > $OUT/prof_fj.log 2>&1
MUMPY_SERIAL=1 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_s16 -- python3 $R/bench.py --full --storage bf16 --steps 10 --warmup 2 --no-cpu-baseline --no-alt > $OUT/prof_s16.log 2>&1
echo "rocprof done"
cd $R
python tools/timeline_gaps.py $OUT/prof_fj 5 > $OUT/timeline_gaps.txt 2>&1
for t in serial fj s16; do
  f=$(find $OUT/prof_$t -name "*kernel_stats.csv" | head -1)
  cp $f $OUT/stats_$t.csv
  python tools/summarize_rocprof.py $f 60 > $OUT/summary_$t.md
  tail -1 $OUT/prof_$t.log > $OUT/benchline_$t.json
  rm -rf $OUT/prof_$t
done
rm -rf $OUT/pmc_bench_FETCH_SIZE $OUT/pmc_bench_WRITE_SIZE
bash tools/pmc_bench.sh > $OUT/pmc_bench.log 2>&1
echo "pmc done"
python tools/phase_timeline.py --graph > $OUT/phase_timeline.txt 2>&1
python tools/gemm_shapes.py > $OUT/gemm_shapes.txt 2>&1
python tools/ln_fold_shapes.py > $OUT/ln_fold_shapes.txt 2>&1
echo "tables done"
python tools/train_ddp_bench.py --batch 2 --math fp32 > $OUT/train_b2_eager.json 2> $OUT/train_final.err
python tools/train_ddp_bench.py --batch 2 --math fp32 --graph --steps 10 > $OUT/train_b2_graph.json 2>> $OUT/train_final.err
python tools/train_ddp_bench.py --batch 2 --math bf16 --graph --steps 10 > $OUT/train_b2_graph_bf16.json 2>> $OUT/train_final.err
python tools/train_ddp_bench.py --batch 2 --math bf16 --graph --steps 10 --train-mode > $OUT/train_b2_graph_bf16_trainmode.json 2>> $OUT/train_final.err
python tools/train_ddp_bench.py --batch 8 --math fp32 > $OUT/train_b8_eager.json 2>> $OUT/train_final.err
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_tr -- python3 $R/tools/train_ddp_bench.py --batch 2 --math fp32 --steps 3 --warmup 1 > $OUT/prof_tr.log 2>&1
cd $R
f=$(find $OUT/prof_tr -name "*kernel_stats.csv" | head -1); python tools/summarize_rocprof.py $f 45 > $OUT/summary_train.md; rm -rf $OUT/prof_tr
tail -2 $OUT/smoke.log
