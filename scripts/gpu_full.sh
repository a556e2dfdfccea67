# full-size headline bench + rocprofv3 evidence (run on the GPU box from the repo root)
mkdir -p gpurun_out
OUT=$_   # the folder made above
python bench.py --steps 20 --warmup 3 --full > $OUT/bench_full.json 2> $OUT/bench_full.err
tail -c 3000 $OUT/bench_full.json
bash scripts/gpu_profile.sh 216 > gpurun_out/profile_full.log 2>&1
tail -40 gpurun_out/prof/summary.txt
