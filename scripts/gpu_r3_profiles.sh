#!/bin/bash
# round 3: the default bench line and the rocprofv3 summaries of every configuration (copied to profiles/r03_*)
mkdir -p gpurun_out/r3p
OUT=$_   # the folder made above
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err; echo "bench rc=$?"
for cfg in ns c2 c3 c4 c5 ns-perturbed; do
  bash scripts/gpu_profile_config.sh $cfg > gpurun_out/r3p/prof_$cfg.log 2>&1
  cp gpurun_out/prof_$cfg/summary.txt gpurun_out/r3p/${cfg}_rocprofv3_summary.txt
  python bench.py --config $cfg --full --no-secondary > $OUT/bench_${cfg}_n1.json 2> $OUT/bench_${cfg}.err
done
python scripts/bench_other_kernels.py > gpurun_out/r3p/other_kernels.jsonl 2> gpurun_out/r3p/other.err
python scripts/check_full_size.py > gpurun_out/r3p/full_size_check.txt 2>&1; tail -3 gpurun_out/r3p/full_size_check.txt
